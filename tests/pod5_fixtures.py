"""POD5 files written for the tests: the embedded Arrow tables by pyarrow
(``pyarrow.ipc.new_file``; extension names as field metadata), the footer flatbuffer and the
framing by hand.  ``python tests/pod5_fixtures.py`` writes the committed files of
tests/golden/pod5 again (README.md there).  Only this module and the pyarrow comparisons of
tests/test_pod5.py need pyarrow; the readers under test never do.
"""
import os
import struct
import sys
import uuid

import numpy as np

ROW_SAMPLES = 4096
SIGNATURE = b'\x8bPOD\r\n\x1a\n'
MARKER = bytes(range(0xA0, 0xB0))           # "chosen per file": this writer's
SIGNAL_TABLE, READS_TABLE, READ_ID_INDEX, OTHER_INDEX, RUN_INFO_TABLE = range(5)


def zstd_compress(data, level=1):
    from vbz_fixtures import zstd_compress as compress
    return compress(bytes(data), level)


# ---- the footer: a flatbuffer, built by hand -----------------------------------------------------
def footer_bytes(contents, software='deepbinner_amd tests', version='0.3.2', identifier=None):
    """table Footer { file_identifier, software, pod5_version: string; contents: [EmbeddedFile] }
    with EmbeddedFile { offset, length: int64; format, content_type: short } for ``contents`` =
    [(offset, length, content_type)], zero-padded to a multiple of 8."""
    buf = bytearray(4)

    def align(n):
        buf.extend(b'\0' * (-len(buf) % n))

    vt_footer = len(buf)
    buf += struct.pack('<HHHHHH', 12, 20, 4, 8, 12, 16)
    footer = len(buf)
    buf += struct.pack('<i', footer - vt_footer) + b'\0' * 16
    struct.pack_into('<I', buf, 0, footer)

    def point(field, target):
        struct.pack_into('<I', buf, field, target - field)

    texts = (identifier or str(uuid.UUID(bytes=MARKER)), software, version)
    for k, text in enumerate(texts):
        align(4)
        point(footer + 4 + 4 * k, len(buf))
        raw = text.encode()
        buf += struct.pack('<I', len(raw)) + raw + b'\0'
    align(4)
    vector = len(buf)
    point(footer + 16, vector)
    buf += struct.pack('<I', len(contents)) + b'\0' * (4 * len(contents))
    align(2)
    vt_entry = len(buf)
    buf += struct.pack('<HHHHHH', 12, 28, 8, 16, 24, 26)
    for k, (offset, length, kind) in enumerate(contents):
        align(8)
        point(vector + 4 + 4 * k, len(buf))
        buf += struct.pack('<iiqqhh', len(buf) - vt_entry, 0, offset, length, 0, kind)
    align(8)
    return bytes(buf)


def frame(tables, marker=MARKER):
    """[(content_type, Arrow IPC file bytes)] -> the bytes of a POD5 file."""
    out = bytearray(SIGNATURE + marker)
    contents = []
    for kind, table in tables:
        contents.append((len(out), len(table), kind))
        out += table + b'\0' * (-len(table) % 8) + marker
    footer = footer_bytes(contents)
    out += b'FOOTER\0\0' + footer + struct.pack('<q', len(footer)) + marker + SIGNATURE
    return bytes(out)


# ---- the tables, by pyarrow ---------------------------------------------------------------------
def _extension(name):
    return {'ARROW:extension:name': name, 'ARROW:extension:metadata': ''}


def _ipc_file(schema, batches):
    import pyarrow as pa
    sink = pa.BufferOutputStream()
    with pa.ipc.new_file(sink, schema) as writer:
        for batch in batches:
            writer.write_batch(batch)
    return sink.getvalue().to_pybytes()


def signal_table(rows, compressed=True, batches=2):
    """rows = [(read id bytes, stored bytes or int16 samples, samples)] -> Arrow IPC file bytes,
    the rows split over ``batches`` record batches."""
    import pyarrow as pa
    kind = pa.large_binary() if compressed else pa.large_list(pa.int16())
    schema = pa.schema([
        pa.field('read_id', pa.binary(16), nullable=False, metadata=_extension('minknow.uuid')),
        pa.field('signal', kind, nullable=False,
                 metadata=_extension('minknow.vbz') if compressed else None),
        pa.field('samples', pa.uint32(), nullable=False)])
    cut = [len(rows) * k // batches for k in range(batches + 1)]
    out = []
    for a, b in zip(cut[:-1], cut[1:]):
        part = rows[a:b]
        signal = [bytes(r[1]) for r in part] if compressed else [np.asarray(r[1], np.int16) for r in part]
        out.append(pa.record_batch([
            pa.array([r[0] for r in part], pa.binary(16)),
            pa.array(signal, kind),
            pa.array([r[2] for r in part], pa.uint32())], schema=schema))
    return _ipc_file(schema, out)


def reads_table(reads):
    """reads = [(read id bytes, [rows of the signal table], num_samples)] -> Arrow IPC file bytes
    with the kinds of columns a real reads table carries around the three that are read: float32,
    uint16, bool, dictionary<int16, utf8> (with its dictionary batch) and a utf8 column in front
    of ``signal``."""
    import pyarrow as pa
    n = len(reads)
    labelled = pa.dictionary(pa.int16(), pa.utf8())
    schema = pa.schema([
        pa.field('read_id', pa.binary(16), nullable=False, metadata=_extension('minknow.uuid')),
        pa.field('tag', pa.utf8()),
        pa.field('signal', pa.list_(pa.uint64()), nullable=False),
        pa.field('channel', pa.uint16(), nullable=False),
        pa.field('pore_type', labelled),
        pa.field('calibration_offset', pa.float32()),
        pa.field('calibration_scale', pa.float32()),
        pa.field('read_number', pa.uint32()),
        pa.field('median_before', pa.float32()),
        pa.field('num_samples', pa.uint64(), nullable=False),
        pa.field('end_reason', labelled),
        pa.field('end_reason_forced', pa.bool_()),
        pa.field('run_info', labelled)])

    def labels(names, picks):
        return pa.DictionaryArray.from_arrays(pa.array(picks, pa.int16()), pa.array(names, pa.utf8()))

    batch = pa.record_batch([
        pa.array([r[0] for r in reads], pa.binary(16)),
        pa.array(['read %d' % k if k % 3 else None for k in range(n)], pa.utf8()),
        pa.array([[int(row) for row in r[1]] for r in reads], pa.list_(pa.uint64())),
        pa.array([(37 * k) % 512 + 1 for k in range(n)], pa.uint16()),
        labels(['not_set', 'r9.4.1'], [k % 2 for k in range(n)]),
        pa.array([-240.0 + k for k in range(n)], pa.float32()),
        pa.array([0.1755 + 0.001 * k for k in range(n)], pa.float32()),
        pa.array([1000 + k for k in range(n)], pa.uint32()),
        pa.array([200.5 + k if k % 2 else None for k in range(n)], pa.float32()),
        pa.array([int(r[2]) for r in reads], pa.uint64()),
        labels(['unknown', 'signal_positive', 'unblock_mux_change'], [k % 3 for k in range(n)]),
        pa.array([k % 2 == 0 for k in range(n)], pa.bool_()),
        labels(['run-0'], [0] * n)], schema=schema)
    return _ipc_file(schema, [batch])


def run_info_table():
    """A table the reader has no use for and must step over."""
    import pyarrow as pa
    schema = pa.schema([pa.field('acquisition_id', pa.utf8()), pa.field('sample_rate', pa.uint16())])
    return _ipc_file(schema, [pa.record_batch([pa.array(['run-0']), pa.array([4000], pa.uint16())],
                                              schema=schema)])


# ---- whole files --------------------------------------------------------------------------------
def rows_of(signal, row_samples=ROW_SAMPLES):
    signal = np.asarray(signal, dtype=np.int16)
    return [signal[a:a + row_samples] for a in range(0, len(signal), row_samples)] or [signal]


def pod5_bytes(reads, compressed=True, level=1, row_samples=ROW_SAMPLES, damage=None, batches=2):
    """reads = [(read id str, int16 signal)] -> the bytes of a POD5 file.  ``damage``: {read
    index: 'cut' (its middle row one data byte short, behind a valid zstd frame) | 'outside' (its
    last row number beyond the signal table)}."""
    from deepbinner_amd import pod5_lite
    damage = damage or {}
    rows, table = [], []
    for k, (read_id, signal) in enumerate(reads):
        raw_id = uuid.UUID(read_id).bytes
        parts = rows_of(signal, row_samples)
        mine = list(range(len(rows), len(rows) + len(parts)))
        for j, part in enumerate(parts):
            if not compressed:
                rows.append((raw_id, part, len(part)))
                continue
            stream = pod5_lite.encode_svb16(part)
            if damage.get(k) == 'cut' and j == len(parts) // 2:
                stream = stream[:-1]
            rows.append((raw_id, zstd_compress(stream, level), len(part)))
        table.append([raw_id, mine, len(signal)])
    for k, how in damage.items():
        if how == 'outside':
            table[k][1][-1] = len(rows) + 5
    return frame([(SIGNAL_TABLE, signal_table(rows, compressed, batches)),
                  (RUN_INFO_TABLE, run_info_table()),
                  (READS_TABLE, reads_table([tuple(r) for r in table]))])


def embedded(path):
    """{content_type: bytes of the embedded Arrow IPC file} of a POD5 file, by the framing of
    DESIGN.md section 36 read in the plainest way (the tests hand these ranges to pyarrow)."""
    data = open(path, 'rb').read()
    length = struct.unpack_from('<q', data, len(data) - 32)[0]
    footer = data[len(data) - 32 - length:len(data) - 32]
    root = struct.unpack_from('<I', footer, 0)[0]
    vt = root - struct.unpack_from('<i', footer, root)[0]
    field = root + struct.unpack_from('<H', footer, vt + 4 + 2 * 3)[0]
    vector = field + struct.unpack_from('<I', footer, field)[0]
    out = {}
    for k in range(struct.unpack_from('<I', footer, vector)[0]):
        at = vector + 4 + 4 * k
        entry = at + struct.unpack_from('<I', footer, at)[0]
        evt = entry - struct.unpack_from('<i', footer, entry)[0]
        offs = struct.unpack_from('<4H', footer, evt + 4)
        offset, size = (struct.unpack_from('<q', footer, entry + o)[0] for o in offs[:2])
        out[struct.unpack_from('<h', footer, entry + offs[3])[0]] = data[offset:offset + size]
    return out


GOLDEN_DAMAGE = {1: 'cut', 4: 'outside'}
TRIM = 8192         # samples kept per end of a long read in the two smaller files


def golden_reads():
    here = os.path.dirname(os.path.abspath(__file__))
    reads = np.load(os.path.join(here, 'golden', 'reads.npz'))
    offsets = reads['offsets']
    return [(str(rid), reads['samples'][offsets[k]:offsets[k + 1]])
            for k, rid in enumerate(reads['read_ids'])]


def trimmed(reads, keep=TRIM):
    """every read longer than 2 * keep cut to its first and last ``keep`` samples: what classify
    looks at (scan_size + half a window from either end) stays"""
    return [(rid, s if len(s) <= 2 * keep else np.concatenate([s[:keep], s[-keep:]]))
            for rid, s in reads]


def golden_files():
    reads = golden_reads()
    return {'golden7.pod5': pod5_bytes(reads, level=19),
            'golden7_uncompressed.pod5': pod5_bytes(trimmed(reads), compressed=False),
            'golden7_damaged.pod5': pod5_bytes(trimmed(reads), level=19, damage=GOLDEN_DAMAGE)}


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    target = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pod5')
    os.makedirs(target, exist_ok=True)
    for name, data in golden_files().items():
        with open(os.path.join(target, name), 'wb') as f:
            f.write(data)
        print(name, len(data))
