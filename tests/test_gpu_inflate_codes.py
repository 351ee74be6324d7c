"""
The inflate kernels (dbh_inflate.hip through the C ABI's dbh_inflate) on the hand-built deflate
streams of tests/deflate_cases.py: the code space of the fixed block, refusals inside the data,
dynamic headers and codes zlib's encoder never writes, stored blocks at every bit position, tokens
placed at the seams of kernel 2's ring, seeded random multi-block streams and every single-bit
flip of six dynamic block headers.  One launch per group of families with all its streams; the
WHOLE output buffer is compared - each stream's bytes, zero-extended to what was wanted, zeros for
a refused stream and between the streams - and every status, under both forms of the launch.
(The same tables on the CPU, through the decoder core compiled for the host:
tests/test_deflate_cases.py.)
"""
import struct
import zlib

import numpy as np
import pytest

import deflate_cases as dc
import shuffle_fixtures as sf
from test_inflate import kernel1, pack_streams      # noqa: F401  (kernel1: both forms of the launch)

pytestmark = pytest.mark.gpu

GROUPS = {'ABCD': 'ABCD', 'E': 'E', 'F': 'F', 'G': 'G'}
_STATUS = {}                  # (form of the launch, group) -> the statuses of that group's own launch


def cases_of(group):
    f = dc.families()
    return [c for family in GROUPS[group] for c in f[family]]


def expected_buffer(items, places, out_bytes):
    """items: [(name, want bytes or None)] -> the whole output buffer as it must be"""
    want = np.zeros(out_bytes, dtype=np.uint8)
    for (name, data), (at, cap) in zip(items, places):
        if data:
            assert len(data) <= cap, name
            want[at:at + len(data)] = np.frombuffer(data, dtype=np.uint8)
    return want


def compare(items, places, out, want, what=''):
    assert out.shape == want.shape
    if np.array_equal(out, want):
        return
    at = int(np.nonzero(out != want)[0][0])
    for (name, _), (start, cap) in zip(items, places):
        if start <= at < start + cap + (cap & 1):
            raise AssertionError('%s%s: first wrong byte at %d of %d wanted' % (what, name, at - start, cap))
    raise AssertionError('%sa wrong byte outside every stream, at %d' % (what, at))


def check_status(cases, status, what=''):
    for (name, _, _, expected), st in zip(cases, status):
        if expected is not None:
            assert st == 0, (what, name, int(st))
        elif name.startswith('G.'):
            assert st != 0, (what, name)
        else:
            assert st == dc.STATUS[name], (what, name, int(st), dc.STATUS[name])


def own_launch(hip, form, group):
    """The group's streams in one launch of their own, checked -> the statuses"""
    if (form, group) not in _STATUS:
        cases = cases_of(group)
        comp, records, out_bytes, places = pack_streams(
            hip, [(stream, wanted, hip.INFLATE_ZLIB) for _, stream, wanted, _ in cases])
        out, status, _ = hip.inflate(comp, records, out_bytes)
        items = [(name, expected) for name, _, _, expected in cases]
        compare(items, places, out, expected_buffer(items, places, out_bytes))
        check_status(cases, status)
        _STATUS[(form, group)] = status.copy()
    return _STATUS[(form, group)]


@pytest.mark.parametrize('group', list(GROUPS))
def test_gpu_inflate_hand_built_streams(hip, kernel1, group):
    cases = cases_of(group)
    status = own_launch(hip, kernel1, group)
    assert len(status) == len(cases) > 0
    refused = sum(1 for c in cases if c[3] is None)
    assert int(np.count_nonzero(status)) == refused


def test_gpu_inflate_hand_built_streams_beside_any_neighbour(hip, kernel1):
    """All families in one launch, in a shuffled order and in the reverse of it, stored-as-is
    streams in between: per stream the bytes and the statuses of the families' own launches."""
    cases, own = [], []
    for group in GROUPS:
        cases += cases_of(group)
        own += list(own_launch(hip, kernel1, group))
    rng = np.random.default_rng(29)
    raws = [dc.random_bytes(rng, n) for n in (0, 1, 77, 5000, 40001)]
    order = list(rng.permutation(len(cases)))
    for k, raw in enumerate(raws):                     # (-1 - k: the k-th stored stream)
        order.insert(int(rng.integers(0, len(order) + 1)), -1 - k)
    for what, sequence in (('shuffled: ', order), ('reversed: ', order[::-1])):
        batch, items, want_status = [], [], []
        for j in sequence:
            if j < 0:
                raw = raws[-1 - j]
                batch.append((raw, len(raw) + 10, hip.INFLATE_STORED))
                items.append(('stored %d' % len(raw), raw))
                want_status.append(0)
            else:
                name, stream, wanted, expected = cases[j]
                batch.append((stream, wanted, hip.INFLATE_ZLIB))
                items.append((name, expected))
                want_status.append(own[j])
        comp, records, out_bytes, places = pack_streams(hip, batch)
        out, status, _ = hip.inflate(comp, records, out_bytes)
        compare(items, places, out, expected_buffer(items, places, out_bytes), what)
        wrong = np.nonzero(status != np.array(want_status, dtype=np.int32))[0]
        assert len(wrong) == 0, (what, [(items[k][0], int(status[k]), int(want_status[k])) for k in wrong[:5]])


def test_gpu_inflate_hand_built_streams_on_the_shuffle_route(hip, kernel1):
    """Streams of C and E as DBH_INFLATE_ZLIB_SHUFFLE (u32 N in front, content of even length): the
    samples shuffle_fixtures.unshuffle makes of zlib's bytes; a refused stream keeps the zlib
    stage's own status."""
    f = dc.families()
    # (the route takes a stream that ENDS with exactly its N bytes: none that is wanted short)
    whole = [c for c in f['C'] + f['E'] if c[3] is not None and len(c[3]) % 2 == 0 and len(c[3]) > 0
             and len(zlib.decompress(c[1])) == len(c[3])]
    picked = [c for c in whole if c[0].startswith('C.')][:6] + [c for c in whole if c[0].startswith('E.')][::70]
    assert sum(1 for c in picked if c[0].startswith('C.')) >= 4 and sum(1 for c in picked if c[0].startswith('E.')) >= 6
    bad = [c for c in f['C'] if c[0] in ('C.hlit287', 'C.repeat16_first', 'C.code_length_code.zeros',
                                         'C.one_distance_code.symbol0.unused_code')]
    assert len(bad) == 4
    batch, items, want_status = [], [], []
    for name, stream, wanted, expected in picked + bad:
        n = len(expected) if expected is not None else wanted & ~1
        batch.append((struct.pack('<I', n) + stream, n + 6, hip.INFLATE_ZLIB_SHUFFLE))
        items.append((name, sf.unshuffle(expected).tobytes() if expected is not None else None))
        want_status.append(0 if expected is not None else dc.STATUS[name])
    comp, records, out_bytes, places = pack_streams(hip, batch)
    out, status, _ = hip.inflate(comp, records, out_bytes)
    compare(items, places, out, expected_buffer(items, places, out_bytes))
    assert list(status) == want_status, list(zip([i[0] for i in items], status, want_status))
