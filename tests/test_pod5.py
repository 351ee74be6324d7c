"""POD5 on the host: ``pod5_lite`` on the committed files of
tests/golden/pod5 against pyarrow reading the same embedded ranges and against the golden reads,
the fixture writer's output read by both, every refusal as one line of error from ``classify``,
the directory listing, ``raw_unit``'s records byte for byte, and ``classify`` on a POD5 file with
the oracle-backed model double (the lists route).  No GPU.  Where pyarrow is absent only the
comparisons with it skip.
"""
import os
import re
import struct
import uuid

import numpy as np
import pytest

import pod5_fixtures as pf
from conftest import GOLD, REPO
from deepbinner_amd import classify, load_fast5s, pod5_lite
from deepbinner_amd import deepbinner as cli

POD5 = os.path.join(GOLD, 'pod5')
FILES = ('golden7.pod5', 'golden7_uncompressed.pod5', 'golden7_damaged.pod5')


def need_pyarrow():
    return pytest.importorskip('pyarrow')


def squiggle(rng, n):
    levels = np.repeat(rng.normal(450, 80, n // 8 + 1), 8)[:n]
    return np.clip(np.rint(levels + rng.normal(0, 8, n)), 0, 2047).astype(np.int16)


def three_reads():
    rng = np.random.default_rng(36)
    return [(str(uuid.UUID(bytes=rng.bytes(16), version=4)), squiggle(rng, n)) for n in (250, 100, 333)]


def golden_signals(name):
    reads = pf.golden_reads()
    return reads if name == 'golden7.pod5' else pf.trimmed(reads)


# ---- the committed files ------------------------------------------------------------------------
def test_the_committed_directory_is_small():
    names = sorted(os.listdir(POD5))
    assert names == ['README.md'] + sorted(FILES)
    assert sum(os.path.getsize(os.path.join(POD5, n)) for n in names) < 400 * 1024


@pytest.mark.parametrize('name', FILES)
def test_tables_against_pyarrow(name):
    pa = need_pyarrow()
    path = os.path.join(POD5, name)
    tables = {kind: pa.ipc.open_file(pa.BufferReader(raw)).read_all()
              for kind, raw in pf.embedded(path).items()}
    assert sorted(tables) == [pf.SIGNAL_TABLE, pf.READS_TABLE, pf.RUN_INFO_TABLE]
    signal, reads = tables[pf.SIGNAL_TABLE], tables[pf.READS_TABLE]
    assert len(signal.column('signal').chunks) == 2          # two record batches
    assert reads.schema.names.index('tag') < reads.schema.names.index('signal')
    assert signal.schema.field('read_id').metadata[b'ARROW:extension:name'] == b'minknow.uuid'
    with pod5_lite.open(path) as pod5:
        assert pod5.read_ids == [str(uuid.UUID(bytes=raw)) for raw in reads.column('read_id').to_pylist()]
        assert pod5.num_samples.tolist() == reads.column('num_samples').to_pylist()
        lists = reads.column('signal').to_pylist()
        assert [pod5.rows(i).tolist() for i in range(len(pod5))] == lists
        counts = signal.column('samples').to_pylist()
        assert [pod5.samples(r) for r in range(len(counts))] == counts
        assert pod5.compressed == (name != 'golden7_uncompressed.pod5')
        stored = signal.column('signal').to_pylist()
        for row, want in enumerate(stored):
            got = pod5.chunk_bytes(row)
            assert got.base is not None                      # a view of the file, no copy
            want = want if pod5.compressed else np.array(want, dtype='<i2').tobytes()
            assert bytes(got) == want, row


@pytest.mark.parametrize('name', FILES)
def test_decoded_signals_are_the_golden_reads(name):
    reads = golden_signals(name)
    with pod5_lite.open(os.path.join(POD5, name)) as pod5:
        assert len(pod5) == 7 and pod5.read_ids == [rid for rid, _ in reads]
        refused = sorted(pf.GOLDEN_DAMAGE) if name == 'golden7_damaged.pod5' else []
        assert np.flatnonzero(pod5.status).tolist() == [k for k in refused
                                                        if pf.GOLDEN_DAMAGE[k] == 'outside']
        for i, (_, want) in enumerate(reads):
            got = pod5_lite.signal(pod5, i)
            if i in refused:
                assert got is None
            else:
                assert got.dtype == np.int16 and np.array_equal(got, want), i
            assert len(pod5.rows(i)) == -(-len(want) // pf.ROW_SAMPLES) >= 2


def test_the_writers_output_is_read_by_pyarrow_and_by_pod5_lite(tmp_path):
    pa = need_pyarrow()
    reads = three_reads()
    for compressed in (True, False):
        path = tmp_path / ('three_%d.pod5' % compressed)
        path.write_bytes(pf.pod5_bytes(reads, compressed=compressed, row_samples=100))
        tables = {k: pa.ipc.open_file(pa.BufferReader(raw)).read_all()
                  for k, raw in pf.embedded(str(path)).items()}
        assert tables[pf.SIGNAL_TABLE].num_rows == 3 + 1 + 4
        assert tables[pf.READS_TABLE].column('pore_type').type == pa.dictionary(pa.int16(), pa.utf8())
        with pod5_lite.open(path) as pod5:
            assert pod5.read_ids == [rid for rid, _ in reads]
            for i, (_, want) in enumerate(reads):
                assert np.array_equal(pod5_lite.signal(pod5, i), want)


# ---- refusals -----------------------------------------------------------------------------------
def refused_files(tmp_path):
    """{what: (path, a word of the reason)}"""
    pa = need_pyarrow()
    reads = three_reads()
    good = pf.pod5_bytes(reads, row_samples=100)
    footer_length_at = len(good) - 32
    cases = {
        'first_signature': (b'\x00' + good[1:], 'signature'),
        'last_signature': (good[:-1] + b'\x00', 'signature'),
        'marker': (good[:8] + bytes(16) + good[24:], 'marker'),
        'footer_length': (good[:footer_length_at] + struct.pack('<q', len(good)) +
                          good[footer_length_at + 8:], 'footer'),
        'footer_magic': (good.replace(b'FOOTER\0\0', b'FOOTER\0\1'), 'FOOTER'),
        'too_short': (good[:40], 'short'),
    }
    rows = [(uuid.UUID(rid).bytes, pf.zstd_compress(pod5_lite.encode_svb16(s)), len(s)) for rid, s in reads]
    table = [(uuid.UUID(rid).bytes, [k], len(s)) for k, (rid, s) in enumerate(reads)]
    cases['no_reads_table'] = (pf.frame([(pf.SIGNAL_TABLE, pf.signal_table(rows))]), 'reads table')
    cases['no_signal_table'] = (pf.frame([(pf.READS_TABLE, pf.reads_table(table))]), 'signal table')
    # a record batch with body compression
    schema = pa.schema([pa.field('read_id', pa.binary(16)), pa.field('signal', pa.large_binary()),
                        pa.field('samples', pa.uint32())])
    batch = pa.record_batch([pa.array([r[0] for r in rows], pa.binary(16)),
                             pa.array([r[1] for r in rows], pa.large_binary()),
                             pa.array([r[2] for r in rows], pa.uint32())], schema=schema)
    sink = pa.BufferOutputStream()
    with pa.ipc.new_file(sink, schema, options=pa.ipc.IpcWriteOptions(compression='zstd')) as writer:
        writer.write_batch(batch)
    cases['compressed_body'] = (pf.frame([(pf.SIGNAL_TABLE, sink.getvalue().to_pybytes()),
                                          (pf.READS_TABLE, pf.reads_table(table))]), 'compress')
    # a column of a type the walk does not know, in front of a wanted one
    schema = pa.schema([pa.field('read_id', pa.binary(16)),
                        pa.field('odd_one', pa.month_day_nano_interval()),
                        pa.field('signal', pa.large_binary()), pa.field('samples', pa.uint32())])
    batch = pa.record_batch([batch.column(0), pa.array([None] * len(rows), pa.month_day_nano_interval()),
                             batch.column(1), batch.column(2)], schema=schema)
    sink = pa.BufferOutputStream()
    with pa.ipc.new_file(sink, schema) as writer:
        writer.write_batch(batch)
    cases['unknown_type'] = (pf.frame([(pf.SIGNAL_TABLE, sink.getvalue().to_pybytes()),
                                       (pf.READS_TABLE, pf.reads_table(table))]), 'odd_one')
    out = {}
    for what, (data, word) in cases.items():
        path = tmp_path / (what + '.pod5')
        path.write_bytes(data)
        out[what] = (str(path), word)
    return out


def test_every_refusal_is_one_line_from_classify(tmp_path, oracle_backend, capsys):
    cases = refused_files(tmp_path)
    assert len(cases) == 10
    for what, (path, word) in cases.items():
        with pytest.raises(pod5_lite.Pod5Error) as refused:
            pod5_lite.open(path)
        assert isinstance(refused.value, OSError), what
        with pytest.raises(SystemExit) as exit_:
            cli.main(['classify', '--rapid', path])
        message = str(exit_.value.code)
        assert message.startswith('Error: ') and '\n' not in message, (what, message)
        assert path in message and word in message, (what, message)
        assert 'Traceback' not in capsys.readouterr().err
    # ... and inside a directory, before anything is classified
    with pytest.raises(SystemExit) as exit_:
        cli.main(['classify', '--rapid', str(tmp_path)])
    assert str(exit_.value.code).startswith('Error: ') and '.pod5' in str(exit_.value.code)


def test_a_file_that_is_not_there_or_empty(tmp_path):
    empty = tmp_path / 'empty.pod5'
    empty.write_bytes(b'')
    for path in (empty, tmp_path / 'nowhere.pod5'):
        with pytest.raises(pod5_lite.Pod5Error) as refused:
            pod5_lite.open(path)
        assert str(path) in str(refused.value) and '\n' not in str(refused.value)


def test_damage_in_the_footers_is_refused_never_raised(tmp_path):
    """three random bytes in the last 6,000 (the tables' Arrow footers and the file's own): the
    file opens, or is refused in one line - no other exception comes out of the reader"""
    data = open(os.path.join(POD5, 'golden7_damaged.pod5'), 'rb').read()
    rng = np.random.default_rng(1)
    path = tmp_path / 'hit.pod5'
    refused = opened = 0
    for _ in range(300):
        hit = bytearray(data)
        for _ in range(3):
            hit[int(rng.integers(len(hit) - 6000, len(hit)))] = int(rng.integers(0, 256))
        path.write_bytes(bytes(hit))
        try:
            pod5_lite.open(path).close()
            opened += 1
        except pod5_lite.Pod5Error as why:
            assert '\n' not in str(why) and str(path) in str(why)
            refused += 1
    assert refused > 50 and opened > 50


def test_footer_fields_at_their_defaults_may_be_absent(tmp_path):
    """a flatbuffer writer leaves out a scalar that has its default value: format 0 and content
    type 0 of the signal table's entry have no slot in a vtable cut behind ``length``"""
    data = bytearray(pf.pod5_bytes(three_reads(), row_samples=100))
    length = struct.unpack_from('<q', data, len(data) - 32)[0]
    at = len(data) - 32 - length
    footer = data[at:at + length]
    vt = footer.index(struct.pack('<HHHHHH', 12, 28, 8, 16, 24, 26))
    # (one vtable serves the three entries: give the signal table's entry, the first, its own)
    first_entry = vt + 12 + (-(vt + 12) % 8)
    own = struct.pack('<HHHH', 8, 28, 8, 16)
    spare = footer.index(b'deepbinner_amd tests')       # eight bytes of the software string
    footer[spare:spare + 8] = own
    struct.pack_into('<i', footer, first_entry, first_entry - spare)
    data[at:at + length] = footer
    path = tmp_path / 'defaults.pod5'
    path.write_bytes(bytes(data))
    with pod5_lite.open(path) as pod5:
        assert len(pod5) == 3 and pod5.compressed


# ---- listing and the other commands -------------------------------------------------------------
def test_directory_listing(tmp_path, capsys):
    for name in ('b.fast5', 'a.pod5', 'c.pod5', 'sub/a.fast5', 'notes.txt'):
        (tmp_path / name).parent.mkdir(exist_ok=True)
        (tmp_path / name).write_bytes(b'')
    plain = load_fast5s.find_all_fast5s(str(tmp_path))
    assert sorted(os.path.relpath(p, str(tmp_path)) for p in plain) == ['b.fast5', 'sub/a.fast5']
    both = load_fast5s.find_all_fast5s(str(tmp_path), verbose=True, pod5=True)
    assert [os.path.relpath(p, str(tmp_path)) for p in both] == ['a.pod5', 'b.fast5', 'c.pod5',
                                                                  'sub/a.fast5']
    assert '2 fast5 and 2 pod5 files found' in capsys.readouterr().err
    # a tree without POD5 files lists what it did, in the order it did
    for name in ('a.pod5', 'c.pod5'):
        (tmp_path / name).unlink()
    assert load_fast5s.find_all_fast5s(str(tmp_path), pod5=True) == plain
    load_fast5s.find_all_fast5s(str(tmp_path), verbose=True, pod5=True)
    assert '2 fast5s found' in capsys.readouterr().err


@pytest.mark.parametrize('command', ['sweep', 'scan', 'locate', 'replay', 'realtime'])
def test_the_other_commands_refuse_a_pod5_path(command, tmp_path, capsys):
    """each command, through the command line, with a real POD5 file: one line, before a model is
    loaded (no model double is installed here: loading one would need a GPU)"""
    import shutil
    path = tmp_path / 'run.pod5'
    shutil.copy(os.path.join(POD5, 'golden7_damaged.pod5'), str(path))
    if command == 'realtime':
        argvs = [['realtime', '--rapid', '--in_dir', str(path), '--out_dir', str(tmp_path / 'out'), '--stop'],
                 # ... and a watched directory that holds POD5 files
                 ['realtime', '--rapid', '--in_dir', str(tmp_path), '--out_dir', str(tmp_path / 'out'),
                  '--stop']]
    else:
        argvs = [[command, '--rapid', str(path)]]
    for argv in argvs:
        with pytest.raises(SystemExit) as exit_:
            cli.main(argv)
        message = str(exit_.value.code)
        assert message.startswith('Error: deepbinner ' + command + ' does not read POD5'), message
        assert '\n' not in message and 'run.pod5' in message
        assert 'Traceback' not in capsys.readouterr().err
    classify.refuse_pod5('/data/run.fast5', command)
    classify.refuse_pod5(str(tmp_path / 'nowhere'), command)


def test_the_product_imports_no_pyarrow_torch_or_h5py():
    offenders = []
    for root, _, names in os.walk(os.path.join(REPO, 'deepbinner_amd')):
        for name in names:
            if name.endswith('.py'):
                with open(os.path.join(root, name)) as f:
                    if re.search(r'^\s*(import|from)\s+(pyarrow|torch|h5py|pod5)\b', f.read(), re.M):
                        offenders.append(name)
    assert not offenders, offenders


# ---- raw units ----------------------------------------------------------------------------------
def expected_unit(reads, mode, first=0, count=None):
    """what raw_unit must hand over for a file of ``reads`` in rows of 100, put together here"""
    chosen = reads[first:None if count is None else first + count]
    comp, records, at = bytearray(), [], 0
    for k, (_, signal) in enumerate(chosen):
        for part in pf.rows_of(signal, 100):
            if mode == pod5_lite.RAW_STORED:
                body = part.astype('<i2').tobytes()
            else:
                stream = pod5_lite.encode_svb16(part)
                body = struct.pack('<I', 2 * len(part)) + (
                    stream if mode == pod5_lite.RAW_SVB16 else pf.zstd_compress(stream))
            records.append((len(comp), len(body), at, 2 * len(part), mode, k))
            comp += body
            at += 2 * len(part)
    offsets = np.concatenate([[0], np.cumsum([len(s) for _, s in chosen])])
    return ([rid for rid, _ in chosen], offsets, bytes(comp) + bytes(64),
            np.array(records, dtype=pod5_lite.RAW_STREAM))


@pytest.mark.parametrize('zstd, compressed', [('host', True), ('gpu', True), ('host', False)])
def test_raw_unit_byte_for_byte(zstd, compressed, tmp_path):
    need_pyarrow()
    reads = three_reads()
    path = tmp_path / 'three.pod5'
    path.write_bytes(pf.pod5_bytes(reads, compressed=compressed, row_samples=100))
    mode = (pod5_lite.RAW_STORED if not compressed else
            pod5_lite.RAW_SVB16 if zstd == 'host' else pod5_lite.RAW_SVB16_ZSTD)
    for first, count in ((0, None), (1, 1), (2, 5)):
        ids, offsets, comp, records = pod5_lite.raw_unit(str(path), first, count, zstd=zstd)
        want = expected_unit(reads, mode, first, count)
        assert ids == want[0] and offsets.tolist() == want[1].tolist() and offsets.dtype == np.int64
        assert comp.dtype == np.uint8 and comp.tobytes() == want[2]
        assert records.dtype == pod5_lite.RAW_STREAM and records.tobytes() == want[3].tobytes()
    from deepbinner_amd import fast5_native
    assert pod5_lite.RAW_STREAM == fast5_native.RAW_STREAM


def test_raw_unit_of_the_damaged_file_and_the_route_flag(monkeypatch):
    ids, offsets, comp, records = pod5_lite.raw_unit(os.path.join(POD5, 'golden7_damaged.pod5'))
    reads = pf.trimmed(pf.golden_reads())
    assert [rid is None for rid in ids] == [k == 4 for k in range(7)]      # rows outside the table
    assert offsets[5] == offsets[4] and 4 not in records['read'].tolist()
    assert set(records['mode'].tolist()) == {pod5_lite.RAW_SVB16}           # (the cut row too: the
    assert offsets[-1] == sum(len(s) for k, (_, s) in enumerate(reads) if k != 4)   # GPU refuses it)
    monkeypatch.delenv('DEEPBINNER_VBZ_ZSTD', raising=False)
    assert pod5_lite.zstd_route() == 'host'
    monkeypatch.setenv('DEEPBINNER_VBZ_ZSTD', 'gpu')
    assert pod5_lite.zstd_route() == 'gpu'
    with pytest.raises(ValueError):
        pod5_lite.raw_unit(os.path.join(POD5, 'golden7.pod5'), zstd='device')


def test_a_frame_without_a_content_size_stays_the_hosts(tmp_path):
    """zstd='gpu': a frame whose header names no content size (written through libzstd's context
    with the content-size flag off) goes out with its zstd stage undone on the host"""
    import ctypes
    need_pyarrow()
    rid, samples = three_reads()[0]
    stream = pod5_lite.encode_svb16(samples)
    lib = ctypes.CDLL('libzstd.so.1')
    lib.ZSTD_createCCtx.restype = ctypes.c_void_p
    lib.ZSTD_CCtx_setParameter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.ZSTD_compress2.restype = ctypes.c_size_t
    lib.ZSTD_compress2.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                   ctypes.c_size_t]
    lib.ZSTD_freeCCtx.argtypes = [ctypes.c_void_p]
    context = lib.ZSTD_createCCtx()
    assert lib.ZSTD_CCtx_setParameter(context, 200, 0) == 0          # ZSTD_c_contentSizeFlag
    room = ctypes.create_string_buffer(len(stream) + 512)
    size = lib.ZSTD_compress2(context, room, len(room), stream, len(stream))
    lib.ZSTD_freeCCtx(context)
    unsized = room.raw[:size]
    assert pod5_lite.frame_content_size(np.frombuffer(unsized, np.uint8)) is None
    assert pod5_lite.frame_content_size(np.frombuffer(pf.zstd_compress(stream), np.uint8)) == len(stream)
    path = tmp_path / 'unsized.pod5'
    raw_id = uuid.UUID(rid).bytes
    path.write_bytes(pf.frame([
        (pf.SIGNAL_TABLE, pf.signal_table([(raw_id, unsized, len(samples))], batches=1)),
        (pf.READS_TABLE, pf.reads_table([(raw_id, [0], len(samples))]))]))
    _, _, comp, records = pod5_lite.raw_unit(str(path), zstd='gpu')
    assert records['mode'].tolist() == [pod5_lite.RAW_SVB16]
    assert comp[:-64].tobytes() == struct.pack('<I', 2 * len(samples)) + stream
    with pod5_lite.open(path) as pod5:
        assert np.array_equal(pod5_lite.signal(pod5, 0), samples)


# ---- the route, and the lists route's units ------------------------------------------------------
def test_pod5_goes_to_the_gpu_unless_it_is_switched_off(monkeypatch):
    """a host with cores to spare keeps fast5 containers to itself (realtime.host_inflate_share);
    POD5 has no thread team to fall back on: only an explicit switch sends it to the host"""
    from deepbinner_amd import containers, realtime
    for name in ('DEEPBINNER_GPU_INFLATE', 'DEEPBINNER_HOST_INFLATE_SHARE'):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(realtime, 'usable_cpus', lambda: 128)
    assert realtime.host_inflate_share(1) == 100 and not containers.pod5_host_only()
    monkeypatch.setenv('DEEPBINNER_HOST_INFLATE_SHARE', '40')
    assert not containers.pod5_host_only()
    monkeypatch.setenv('DEEPBINNER_HOST_INFLATE_SHARE', '100')
    assert containers.pod5_host_only()
    monkeypatch.setenv('DEEPBINNER_GPU_INFLATE', '1')
    assert not containers.pod5_host_only()
    monkeypatch.setenv('DEEPBINNER_GPU_INFLATE', '0')
    assert containers.pod5_host_only()


def test_the_lists_route_hands_units_on_as_they_are_decoded(monkeypatch):
    """a unit per --batch_size reads, each yielded before the next read is decoded"""
    import argparse
    from deepbinner_amd import containers
    decoded = []
    real = pod5_lite.signal
    monkeypatch.setattr(pod5_lite, 'signal', lambda pod5, i: decoded.append(i) or real(pod5, i))
    units = containers.Units(argparse.Namespace(batch_size=3), 1024, None, 13)
    seen = []
    for unit in containers.pod5_chunks([os.path.join(POD5, 'golden7_damaged.pod5')], units):
        seen.append((list(unit.ids), unit.last, len(decoded)))
    reads = [rid for rid, _ in pf.golden_reads()]
    kept = [rid for k, rid in enumerate(reads) if k not in pf.GOLDEN_DAMAGE]
    assert [ids for ids, _, _ in seen] == [kept[:3], kept[3:]]
    assert [last for _, last, _ in seen] == [False, True]
    assert [n for _, _, n in seen] == [4, 7]        # (reads 0..3 decoded - read 1 refused - then the rest)


# ---- classify, on the lists route with the model double -----------------------------------------
def run(argv, capsys):
    capsys.readouterr()
    cli.main(['classify'] + [str(a) for a in argv])
    done = capsys.readouterr()
    lines = done.out.splitlines()
    return lines[0], lines[1:], done.err


def test_classify_prints_the_golden_calls(oracle_backend, gold, capsys):
    want = dict(zip(gold['read_ids'], gold['calls']['SQK-RBK004_read_starts/start'][:7]))
    header, rows, err = run(['--rapid', os.path.join(POD5, 'golden7.pod5')], capsys)
    assert header == 'read_ID\tbarcode_call'
    assert [row.split('\t')[0] for row in rows] == gold['read_ids']
    assert {row.split('\t')[0]: row.split('\t')[1] for row in rows} == want
    assert 'Classifying fast5s: 1 / 1' in err and 'Barcode     Count' in err and 'Warning' not in err
    _, damaged, err = run(['--rapid', os.path.join(POD5, 'golden7_damaged.pod5')], capsys)
    skipped = [gold['read_ids'][k] for k in sorted(pf.GOLDEN_DAMAGE)]
    assert damaged == [row for row in rows if row.split('\t')[0] not in skipped]
    assert err.count('Warning: skipping read') == 2 and all(rid in err for rid in skipped)
