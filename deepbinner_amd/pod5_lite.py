"""
A reader for POD5 files - ONT's current raw-signal container - in pure Python and NumPy, the way
``hdf5_lite`` reads fast5 without h5py: no ``pod5`` library, no pyarrow.  The format as this
reader takes it is DESIGN.md section 36: a small framing (signature, a per-file marker, a
flatbuffer footer read from the file's end) around embedded Arrow IPC files, of which the signal
table and the reads table are read and every other one is skipped.  Of Arrow it knows what these
two tables use: the IPC footer, the record batch messages, and where a named column's buffers lie,
found by walking the schema and counting each preceding field's buffers by its type.

A read's signal is stored as rows of the signal table, each compressed on its own: a zstd frame
(undone through the system's ``libzstd.so.1`` by ctypes, as ``hdf5_lite`` does for fast5's VBZ)
around the 16-bit streamvbyte code "svb16" (``decode_svb16`` / ``encode_svb16``: the NumPy
restatement of csrc/dbh_svb16_core.h).  ``raw_unit`` hands a run of reads to the unit pipeline
(containers.py) as the GPU decodes them: one ``dbh_inflate_stream`` record per row.

**What this is held to:** the Arrow tables to pyarrow (tests/test_pod5.py), the framing, the footer
and the svb16 code to the published specification as DESIGN.md restates it.  Nothing has been read
here that the ``pod5`` library or MinKNOW wrote.
"""

import os
import struct
import uuid
from concurrent.futures import ThreadPoolExecutor

import numpy as np

SIGNATURE = b'\x8bPOD\r\n\x1a\n'
FOOTER_MAGIC = b'FOOTER\x00\x00'
ARROW_MAGIC = b'ARROW1'
SIGNAL_TABLE, READS_TABLE = 0, 1            # EmbeddedFile.content_type
# the modes of a raw record (include/deepbinner_hip.h; fast5_native.RAW_*)
RAW_STORED, RAW_SVB16, RAW_SVB16_ZSTD = 1, 6, 7
# read status, in fast5_native's numbering: readable / its rows are not what the reads table says
OK, ERR_FORMAT = 0, 2


class Pod5Error(OSError):
    """A file this reader refuses; the message is one line and names the file."""


# ---- svb16: ceil(n/8) key bytes (bit i & 7 of byte i >> 3: value i takes two bytes), data bytes ----
def encode_svb16(samples):
    """int16 samples -> the svb16 stream of their zigzagged 16-bit deltas (fixtures and tools)."""
    x = np.asarray(samples, dtype=np.int16).view(np.uint16)
    n = len(x)
    delta = np.diff(np.concatenate([np.zeros(1, dtype=np.uint16), x])).astype(np.uint16)
    v = ((delta << np.uint16(1)) ^ (np.uint16(0) - (delta >> np.uint16(15)))).astype(np.uint16)
    two = v > 0xFF
    keys = np.packbits(two, bitorder='little')
    pairs = v.astype('<u2').view(np.uint8).reshape(-1, 2)
    take = np.ones((n, 2), dtype=bool)
    take[:, 1] = two
    return keys.tobytes() + pairs[take].tobytes()


def decode_svb16(stream, n):
    """The svb16 stream of n values -> int16 samples, vectorised; None if the key bytes or the
    data they call for do not end exactly where ``stream`` does.  The unused bits of the last key
    byte are not looked at."""
    arr = np.frombuffer(stream, dtype=np.uint8)
    n = int(n)
    n_keys = (n + 7) // 8
    if n < 0 or n_keys > len(arr):
        return None
    two = np.unpackbits(arr[:n_keys], bitorder='little')[:n].astype(np.int64)
    data = arr[n_keys:]
    if n + int(two.sum()) != len(data):
        return None
    starts = np.arange(n, dtype=np.int64) + np.cumsum(two) - two
    padded = np.concatenate([data, np.zeros(1, dtype=np.uint8)]).astype(np.uint16)
    v = padded[starts] | ((padded[starts + 1] << np.uint16(8)) * two.astype(np.uint16))
    delta = (v >> np.uint16(1)) ^ (np.uint16(0) - (v & np.uint16(1)))
    return np.cumsum(delta, dtype=np.uint16).view(np.int16)


# ---- flatbuffers, read by hand: tables through their vtables, no schema compiler -----------------
class _Table:
    """One flatbuffer table at ``pos`` of ``buf``; field k by its number in the schema."""
    __slots__ = ('buf', 'pos', 'vt', 'vt_size')

    def __init__(self, buf, pos):
        if pos < 0 or pos + 4 > len(buf):
            raise ValueError('table outside the buffer')
        vt = pos - struct.unpack_from('<i', buf, pos)[0]
        if vt < 0 or vt + 4 > len(buf):
            raise ValueError('vtable outside the buffer')
        self.buf, self.pos, self.vt = buf, pos, vt
        self.vt_size = struct.unpack_from('<H', buf, vt)[0]
        if vt + self.vt_size > len(buf):
            raise ValueError('vtable outside the buffer')

    @classmethod
    def root(cls, buf):
        return cls(buf, struct.unpack_from('<I', buf, 0)[0])

    def _at(self, k):
        slot = 4 + 2 * k
        if slot + 2 > self.vt_size:
            return 0
        off = struct.unpack_from('<H', self.buf, self.vt + slot)[0]
        return self.pos + off if off else 0

    def scalar(self, k, fmt, default=0):
        at = self._at(k)
        return struct.unpack_from(fmt, self.buf, at)[0] if at else default

    def _indirect(self, k):
        at = self._at(k)
        if not at:
            return 0
        to = at + struct.unpack_from('<I', self.buf, at)[0]
        if to + 4 > len(self.buf):
            raise ValueError('offset outside the buffer')
        return to

    def table(self, k):
        to = self._indirect(k)
        return _Table(self.buf, to) if to else None

    def string(self, k):
        to = self._indirect(k)
        if not to:
            return None
        size = struct.unpack_from('<I', self.buf, to)[0]
        if to + 4 + size > len(self.buf):
            raise ValueError('string outside the buffer')
        return bytes(self.buf[to + 4:to + 4 + size]).decode()

    def vector(self, k):
        """-> (position of element 0, count); (0, 0) if absent"""
        to = self._indirect(k)
        if not to:
            return 0, 0
        return to + 4, struct.unpack_from('<I', self.buf, to)[0]

    def tables(self, k):
        first, count = self.vector(k)
        if first + 4 * count > len(self.buf):
            raise ValueError('vector outside the buffer')
        out = []
        for j in range(count):
            at = first + 4 * j
            out.append(_Table(self.buf, at + struct.unpack_from('<I', self.buf, at)[0]))
        return out

    def structs(self, k, dtype):
        first, count = self.vector(k)
        if first + dtype.itemsize * count > len(self.buf):
            raise ValueError('vector outside the buffer')
        return np.frombuffer(self.buf, dtype=dtype, count=count, offset=first)


# ---- Arrow IPC: what the signal and reads tables use ---------------------------------------------
# Type (Schema.fbs): the union's numbers
(_T_NULL, _T_INT, _T_FLOAT, _T_BINARY, _T_UTF8, _T_BOOL, _T_DECIMAL, _T_DATE, _T_TIME, _T_TIMESTAMP,
 _T_INTERVAL, _T_LIST, _T_STRUCT, _T_UNION, _T_FIXED_BINARY, _T_FIXED_LIST, _T_MAP, _T_DURATION,
 _T_LARGE_BINARY, _T_LARGE_UTF8, _T_LARGE_LIST) = range(1, 22)
_BLOCK = np.dtype([('offset', '<i8'), ('meta', '<i4'), ('pad', '<i4'), ('body', '<i8')])
_BUFFER = np.dtype([('offset', '<i8'), ('length', '<i8')])


class _Field:
    """A field of an Arrow schema: name, type number, what the type says (bit width, signedness,
    byte width), children, whether it is dictionary-encoded, its extension name."""

    def __init__(self, table):
        self.name = table.string(0) or ''
        self.kind = table.scalar(2, '<B')
        detail = table.table(3)
        self.bits = self.signed = self.width = None
        if self.kind == _T_INT and detail is not None:
            self.bits, self.signed = detail.scalar(0, '<i'), bool(detail.scalar(1, '<B'))
        if self.kind == _T_FIXED_BINARY and detail is not None:
            self.width = detail.scalar(0, '<i')
        self.dictionary = table.table(4) is not None
        self.children = [_Field(child) for child in table.tables(5)]
        self.extension = None
        for pair in table.tables(6):
            if pair.string(0) == 'ARROW:extension:name':
                self.extension = pair.string(1)

    def n_buffers(self):
        """How many buffers of a record batch this field and its children take, in the depth-first
        order of the schema; ValueError(the field's name) for a type this walk does not know."""
        if self.dictionary:                 # its index type's: validity, data
            return 2
        kind = self.kind
        if kind == _T_NULL:
            return 0
        if kind in (_T_INT, _T_FLOAT, _T_BOOL, _T_DECIMAL, _T_DATE, _T_TIME, _T_TIMESTAMP,
                    _T_DURATION, _T_FIXED_BINARY):
            return 2
        if kind in (_T_BINARY, _T_UTF8, _T_LARGE_BINARY, _T_LARGE_UTF8):
            return 3
        if kind in (_T_LIST, _T_LARGE_LIST, _T_MAP):        # validity, offsets, then the child
            return 2 + sum(child.n_buffers() for child in self.children)
        if kind in (_T_STRUCT, _T_FIXED_LIST):              # validity, then the children
            return 1 + sum(child.n_buffers() for child in self.children)
        raise ValueError(self.name)


class _ArrowFile:
    """One embedded Arrow IPC file, bytes [start, start + size) of ``data``: its schema and the
    columns of its record batches as views of ``data``."""

    def __init__(self, data, start, size, what):
        self.data, self.start, self.what = data, start, what
        end = start + size
        head = bytes(data[start:start + 6]) if size >= 6 else b''
        # ARROW1\0\0 | messages | footer | int32 footer length | ARROW1
        if size < 8 + 4 + 6 or head != ARROW_MAGIC or bytes(data[end - 6:end]) != ARROW_MAGIC:
            raise ValueError('the {} is not an Arrow IPC file'.format(what))
        footer_size = struct.unpack_from('<i', data, end - 10)[0]
        if footer_size <= 0 or footer_size > size - 18:
            raise ValueError('the {} has an impossible Arrow footer'.format(what))
        footer = _Table.root(data[end - 10 - footer_size:end - 10])
        schema = footer.table(1)
        if schema is None:
            raise ValueError('the {} has no schema'.format(what))
        self.fields = [_Field(f) for f in schema.tables(1)]
        self.blocks = footer.structs(3, _BLOCK)
        self.size = size

    def field(self, name):
        for k, f in enumerate(self.fields):
            if f.name == name:
                return k, f
        raise ValueError('the {} has no column {!r}'.format(self.what, name))

    def first_buffer(self, index):
        try:
            return sum(f.n_buffers() for f in self.fields[:index])
        except ValueError as unknown:
            raise ValueError('the {} has a column of a type this reader does not know: {!r}'
                             .format(self.what, str(unknown))) from None

    def batches(self):
        """-> [(length, buffers as absolute (offset, length) pairs)] per record batch"""
        out = []
        for block in self.blocks:
            at = self.start + int(block['offset'])
            meta, body = int(block['meta']), int(block['body'])
            if (int(block['offset']) < 0 or meta < 8 or body < 0 or
                    int(block['offset']) + meta + body > self.size):
                raise ValueError('the {} has a record batch outside itself'.format(self.what))
            word = struct.unpack_from('<I', self.data, at)[0]
            skip = 8 if word == 0xFFFFFFFF else 4       # (before Arrow 0.15: no continuation word)
            message = _Table.root(self.data[at + skip:at + meta])
            if message.scalar(1, '<B') != 3:            # MessageHeader.RecordBatch
                raise ValueError('the {} lists a message that is no record batch'.format(self.what))
            batch = message.table(2)
            if batch is None:
                raise ValueError('the {} has a record batch message without a header'.format(self.what))
            if batch.table(3) is not None:
                raise ValueError('the {} has compressed record batches (Arrow body compression), '
                                 'which this reader does not undo'.format(self.what))
            buffers = batch.structs(2, _BUFFER)
            base = at + meta
            absolute = []
            for b in buffers:
                off, size = int(b['offset']), int(b['length'])
                if off < 0 or size < 0 or off + size > body:
                    raise ValueError('the {} has a buffer outside its batch'.format(self.what))
                absolute.append((base + off, size))
            out.append((int(batch.scalar(0, '<q')), absolute))
        return out

    def view(self, where, dtype, count):
        offset, size = where
        dtype = np.dtype(dtype)
        if count * dtype.itemsize > size:
            raise ValueError('the {} has a buffer shorter than its rows'.format(self.what))
        return np.frombuffer(self.data, dtype=dtype, count=count, offset=offset)


def _is_uint(field, bits):
    return field.kind == _T_INT and field.bits == bits and not field.signed and not field.dictionary


class Pod5:
    """One open POD5 file.  ``read_ids`` (the 16 stored bytes as a UUID string each),
    ``num_samples`` (uint64 per read), ``rows(i)`` (read i's rows of the signal table, in order),
    ``status`` (int32 per read: non-zero where the rows are outside the table or their samples do
    not add up to num_samples), ``chunk_bytes(row)`` (a view of the stored bytes, no copy),
    ``samples(row)``, ``compressed`` (whether rows are `minknow.vbz` values or plain int16)."""

    def __init__(self, path):
        self.path = str(path)
        try:
            size = os.path.getsize(self.path)
            self.data = np.memmap(self.path, dtype=np.uint8, mode='r') if size else \
                np.zeros(0, dtype=np.uint8)
        except OSError as failed:
            raise Pod5Error('{}: {}'.format(self.path, failed.strerror or failed)) from None
        try:
            self._open()
        except (ValueError, struct.error, IndexError, OverflowError, RecursionError, AttributeError,
                TypeError, MemoryError) as refused:
            raise Pod5Error('{} is not a POD5 file this reader takes: {}'
                            .format(self.path, refused)) from None

    def _open(self):
        data = self.data
        size = len(data)
        # signature | marker | ... | FOOTER\0\0 | footer | int64 length | marker | signature
        if size < 8 + 16 + 8 + 8 + 16 + 8:
            raise ValueError('too short')
        if bytes(data[:8]) != SIGNATURE:
            raise ValueError('no signature at its start')
        if bytes(data[size - 8:]) != SIGNATURE:
            raise ValueError('no signature at its end')
        if bytes(data[size - 24:size - 8]) != bytes(data[8:24]):
            raise ValueError('the section markers at its start and end differ')
        length = struct.unpack_from('<q', data, size - 32)[0]
        footer_at = size - 32 - length
        if length <= 0 or length % 8 or footer_at - 8 < 24:
            raise ValueError('a footer length of {} bytes'.format(length))
        if bytes(data[footer_at - 8:footer_at]) != FOOTER_MAGIC:
            raise ValueError('no FOOTER magic in front of its footer')
        footer = _Table.root(data[footer_at:footer_at + length])
        embedded = {}
        for entry in footer.tables(3):
            offset, extent = entry.scalar(0, '<q'), entry.scalar(1, '<q')
            kind = entry.scalar(3, '<h')
            if kind in (SIGNAL_TABLE, READS_TABLE) and kind not in embedded:
                if entry.scalar(2, '<h') != 0:
                    raise ValueError('an embedded table that is not FeatherV2')
                if offset < 24 or extent < 0 or offset + extent > footer_at - 8:
                    raise ValueError('an embedded table outside the file')
                embedded[kind] = (offset, extent)
        if SIGNAL_TABLE not in embedded:
            raise ValueError('no signal table')
        if READS_TABLE not in embedded:
            raise ValueError('no reads table')
        self._signal_table(_ArrowFile(data, *embedded[SIGNAL_TABLE], 'signal table'))
        self._reads_table(_ArrowFile(data, *embedded[READS_TABLE], 'reads table'))

    def _signal_table(self, table):
        k_signal, signal = table.field('signal')
        k_samples, samples = table.field('samples')
        if signal.kind == _T_LARGE_BINARY:
            self.compressed = True
        elif (signal.kind == _T_LARGE_LIST and len(signal.children) == 1 and
              signal.children[0].kind == _T_INT and signal.children[0].bits == 16 and
              signal.children[0].signed):
            self.compressed = False
        else:
            raise ValueError("the signal table's signal column is neither large_binary nor "
                             "large_list<int16>")
        if not _is_uint(samples, 32):
            raise ValueError("the signal table's samples column is not uint32")
        b_signal, b_samples = table.first_buffer(k_signal), table.first_buffer(k_samples)
        starts, sizes, counts = [], [], []
        for length, buffers in table.batches():
            offsets = table.view(buffers[b_signal + 1], '<i8', length + 1).astype(np.int64)
            # large_binary: validity, offsets, data; large_list: validity, offsets, child validity, data
            where = buffers[b_signal + 2 if self.compressed else b_signal + 3]
            scale = 1 if self.compressed else 2
            if length and (offsets[0] < 0 or (np.diff(offsets) < 0).any() or
                           int(offsets[-1]) * scale > where[1]):
                raise ValueError('the signal table has rows outside their buffer')
            starts.append(where[0] + offsets[:-1] * scale)
            sizes.append(np.diff(offsets) * scale)
            counts.append(table.view(buffers[b_samples + 1], '<u4', length))
        self.row_start = np.concatenate(starts) if starts else np.zeros(0, dtype=np.int64)
        self.row_bytes = np.concatenate(sizes) if sizes else np.zeros(0, dtype=np.int64)
        self.row_samples = (np.concatenate(counts) if counts else np.zeros(0)).astype(np.int64)
        if not self.compressed and (self.row_bytes != 2 * self.row_samples).any():
            # (an uncompressed row is its samples: the list's length has the last word)
            self.row_samples = self.row_bytes // 2

    def _reads_table(self, table):
        k_id, read_id = table.field('read_id')
        k_signal, signal = table.field('signal')
        k_count, count = table.field('num_samples')
        if read_id.kind != _T_FIXED_BINARY or read_id.width != 16:
            raise ValueError("the reads table's read_id column is not fixed_size_binary[16]")
        if signal.kind != _T_LIST or len(signal.children) != 1 or not _is_uint(signal.children[0], 64):
            raise ValueError("the reads table's signal column is not list<uint64>")
        if not _is_uint(count, 64):
            raise ValueError("the reads table's num_samples column is not uint64")
        b_id, b_signal, b_count = (table.first_buffer(k) for k in (k_id, k_signal, k_count))
        ids, lists, rows, counts = [], [np.zeros(1, dtype=np.int64)], [], []
        total = 0
        for length, buffers in table.batches():
            ids.append(table.view(buffers[b_id + 1], 'V16', length))
            offsets = table.view(buffers[b_signal + 1], '<i4', length + 1).astype(np.int64)
            if length and (offsets[0] < 0 or (np.diff(offsets) < 0).any()):
                raise ValueError('the reads table has row lists that run backwards')
            values = table.view(buffers[b_signal + 3], '<u8', int(offsets[-1]) if length else 0)
            first = int(offsets[0]) if length else 0
            rows.append(values[first:])
            lists.append(offsets[1:] - first + total)
            total += len(values) - first
            counts.append(table.view(buffers[b_count + 1], '<u8', length))
        raw = np.concatenate(ids) if ids else np.zeros(0, dtype='V16')
        self.read_ids = [str(uuid.UUID(bytes=r.tobytes())) for r in raw]
        self.num_samples = np.concatenate(counts) if counts else np.zeros(0, dtype=np.uint64)
        self._list = np.concatenate(lists)
        self._rows = np.concatenate(rows) if rows else np.zeros(0, dtype=np.uint64)
        # a read whose rows are outside the table, or do not add up to num_samples, is refused
        outside = self._rows >= np.uint64(len(self.row_samples))
        inside = np.where(outside, 0, self._rows).astype(np.int64)
        held = np.where(outside, 0, self.row_samples[inside] if len(self.row_samples) else 0)
        sums = np.concatenate([[0], np.cumsum(held)])
        bad = np.concatenate([[0], np.cumsum(outside)])
        lo, hi = self._list[:-1], self._list[1:]
        wrong = ((bad[hi] - bad[lo]) != 0) | ((sums[hi] - sums[lo]) != self.num_samples.astype(np.int64))
        self.status = np.where(wrong, ERR_FORMAT, OK).astype(np.int32)

    def __len__(self):
        return len(self.read_ids)

    def rows(self, i):
        return self._rows[self._list[i]:self._list[i + 1]].astype(np.int64)

    def samples(self, row):
        return int(self.row_samples[row])

    def chunk_bytes(self, row):
        start = int(self.row_start[row])
        return self.data[start:start + int(self.row_bytes[row])]

    def close(self):
        self.data = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def open(path):                     # noqa: A001 (the module's entry, as hdf5_lite.File is its)
    """-> Pod5; Pod5Error (an OSError, one line, naming the file) for a file this reader refuses."""
    return Pod5(path)


def is_pod5(path):
    return str(path).endswith('.pod5')


# ---- the zstd stage on the host ------------------------------------------------------------------
def _zstd():
    from . import hdf5_lite
    lib = hdf5_lite._zstd()
    if lib is None:
        raise Pod5Error('libzstd.so.1 is needed to read compressed POD5 signal on the host')
    return lib


def frame_content_size(frame):
    """What the zstd frame header says its content is long, or None if it does not say."""
    lib = _zstd()
    frame = np.ascontiguousarray(frame, dtype=np.uint8)
    size = lib.ZSTD_getFrameContentSize(frame.ctypes.data, len(frame))
    return None if size >= (1 << 64) - 2 else int(size)


def unzstd(frame, n):
    """The zstd frame of one row of n samples -> its svb16 bytes (uint8 array); None where the
    frame names a content size that n values cannot have, or libzstd refuses it.  A frame that
    names none is decoded into the most that n values can take."""
    lib = _zstd()
    frame = np.ascontiguousarray(frame, dtype=np.uint8)
    size = frame_content_size(frame)
    n_keys = (n + 7) // 8
    if size is not None and not n_keys + n <= size <= n_keys + 2 * n:
        return None
    room = n_keys + 2 * n if size is None else size
    out = np.empty(max(room, 1), dtype=np.uint8)
    got = lib.ZSTD_decompress(out.ctypes.data, room, frame.ctypes.data, len(frame))
    if lib.ZSTD_isError(got) or (size is not None and got != size):
        return None
    return out[:got]


def row_signal(pod5, row):
    """One row of the signal table -> int16 samples, or None if its bytes are refused."""
    n, stored = pod5.samples(row), pod5.chunk_bytes(row)
    if not pod5.compressed:
        return np.array(stored).view('<i2') if len(stored) == 2 * n else None
    packed = unzstd(stored, n)
    return None if packed is None else decode_svb16(packed, n)


def signal(pod5, i):
    """Read i's whole signal as int16, decoded on the host; None for a read that is refused (its
    rows are not what the reads table says, or a row's bytes do not decode)."""
    if pod5.status[i] != OK:
        return None
    parts = [row_signal(pod5, int(row)) for row in pod5.rows(i)]
    if any(part is None for part in parts):
        return None
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int16)


# ---- a run of reads as the GPU takes it ----------------------------------------------------------
RAW_STREAM = np.dtype([('comp_offset', '<i8'), ('comp_bytes', '<i8'), ('out_offset', '<i8'),
                       ('out_bytes', '<i8'), ('mode', '<i4'), ('read', '<i4')])
READS_PER_UNIT = 4000               # a POD5 unit is at most a container's worth of reads


def zstd_route():
    """DEEPBINNER_VBZ_ZSTD, as for fast5: 'gpu' leaves the rows' zstd frames to the device."""
    route = os.environ.get('DEEPBINNER_VBZ_ZSTD') or 'host'
    if route not in ('host', 'gpu'):
        raise ValueError("DEEPBINNER_VBZ_ZSTD must be 'host' or 'gpu', not {!r}".format(route))
    return route


def raw_unit(path, first=0, count=None, zstd='host', threads=0):
    """Reads [first, first + count) of a POD5 file (a path or an open ``Pod5``) as a raw unit ->
    (ids, offsets, comp, records): ``offsets`` in samples (count + 1), ``comp`` the rows' bytes
    with 64 bytes of padding behind them, ``records`` one RAW_STREAM per signal row.  A compressed
    row has its 4-byte prefix (u32 LE 2 n) in front of its bytes: mode SVB16 with the zstd frame
    undone here by a small thread pool, or with ``zstd='gpu'`` mode SVB16_ZSTD with the frame as
    stored - unless its header names no content size or one that n values cannot have: that row
    stays the host's.  Uncompressed files give STORED records.  A refused read (``status``) has id
    None, no samples and no record."""
    if zstd not in ('host', 'gpu'):
        raise ValueError("zstd must be 'host' or 'gpu', not {!r}".format(zstd))
    pod5 = path if isinstance(path, Pod5) else Pod5(path)
    n_reads = len(pod5)
    last = n_reads if count is None else min(n_reads, first + int(count))
    reads = range(int(first), last)
    ids = [pod5.read_ids[i] if pod5.status[i] == OK else None for i in reads]
    lengths = [int(pod5.num_samples[i]) if pod5.status[i] == OK else 0 for i in reads]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    plan = []                       # (read of the unit, row, out_offset in bytes)
    for k, i in enumerate(reads):
        if pod5.status[i] != OK:
            continue
        at = 2 * int(offsets[k])
        for row in pod5.rows(i).tolist():
            plan.append((k, row, at))
            at += 2 * pod5.samples(row)

    def stage(item):
        _, row, _ = item
        stored, n = pod5.chunk_bytes(row), pod5.samples(row)
        if not pod5.compressed:
            return RAW_STORED, stored
        if zstd == 'gpu':
            size = frame_content_size(stored)
            n_keys = (n + 7) // 8
            if size is not None and n_keys <= size <= n_keys + 2 * n:
                return RAW_SVB16_ZSTD, stored
        packed = unzstd(stored, n)
        # (a frame the host refuses goes out as it is: the device refuses it too, and the read is
        # read again by the host, which then says so)
        return (RAW_SVB16, packed) if packed is not None else (RAW_SVB16_ZSTD, stored)

    if pod5.compressed and zstd == 'host' and len(plan) > 1:
        from .misc import usable_cpus
        workers = int(threads) if threads and int(threads) > 0 else max(1, min(8, usable_cpus()))
        with ThreadPoolExecutor(max_workers=workers, thread_name_prefix='deepbinner-pod5') as pool:
            staged = list(pool.map(stage, plan))
    else:
        staged = [stage(item) for item in plan]
    prefix = 4 if pod5.compressed else 0
    records = np.zeros(len(plan), dtype=RAW_STREAM)
    sizes = np.array([prefix + len(body) for _, body in staged], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    comp = np.zeros(int(starts[-1]) + 64, dtype=np.uint8)
    for j, ((k, row, at), (mode, body)) in enumerate(zip(plan, staged)):
        n, start = pod5.samples(row), int(starts[j])
        if prefix:
            comp[start:start + 4] = np.frombuffer(struct.pack('<I', (2 * n) & 0xFFFFFFFF), np.uint8)
        comp[start + prefix:start + prefix + len(body)] = body
        records[j] = (start, sizes[j], at, 2 * n, mode, k)
    return ids, offsets, comp, records
