"""
The hand-built deflate streams of tests/deflate_cases.py (what zlib's encoder never writes, header
refusals, tokens at the resolve kernel's seams, random multi-block streams, header mutants) held to
zlib, and the decoder core compiled for the host (oracle/_build/inflate_host_test: the one-lane
decoder, the wave form with every table answer checked against the canonical one, and the model of
kernel 2's schedule) held to the tables.  The kernels themselves: tests/test_gpu_inflate_codes.py.
"""
import zlib

import pytest

import deflate_cases as dc
from test_inflate import needs_harness, run_harness

FAMILIES = 'ABCDEFG'


@pytest.mark.parametrize('family', FAMILIES)
def test_the_tables_hold_against_zlib(family):
    """zlib.decompress of every stream gives the table's bytes, or raises where the table has a
    refusal; no family is without the verdicts it is there for."""
    cases = dc.families()[family]
    n_ok, n_bad = dc.check_against_zlib(cases)
    assert n_ok + n_bad == len(cases)
    assert (n_ok > 0 or family == 'G') and (n_bad > 0 or family in 'AEF')
    for name, _, wanted, expected in cases:
        assert expected is None or len(expected) <= wanted
        assert (name in dc.STATUS) == (expected is None and family != 'G'), name


def test_the_tables_hold_what_they_are_to_hold():
    f = dc.families()
    names = {c[0] for cases in f.values() for c in cases}
    assert len(f['A']) == 257 * 11 + (30 * 2 - 4) * 2
    assert len(f['F']) == 150 and len(f['G']) == 6 * dc.G_BITS
    assert sum(1 for c in f['F'] if len(zlib.decompress(c[1])) > c[2]) >= 25
    for p in dc.E_PREFIXES:
        for dist in (4095, 4096, 4097, dc.RING - 8, dc.RING - 1, dc.RING, dc.RING + 1, dc.RING + 8, p - 1, p, 32768):
            if dist <= min(p, 32768):
                assert all('E.p%d.len%d.d%d' % (p, length, dist) in names for length in dc.E_LENGTHS)
    for name in ('C.repeat16_first', 'C.hlit287', 'C.hlit288', 'C.hdist31', 'C.hdist32', 'C.hclen4'):
        assert dc.STATUS[name] == dc.BAD_CODES


@needs_harness
@pytest.mark.parametrize('family', FAMILIES)
def test_decoder_core_on_hand_built_streams(family, tmp_path):
    """Status, bytes, `ended` and `adler_ok` of every case as in test_inflate.py's two harness
    tests; a refused case of A-F with exactly the table's status."""
    cases = dc.families()[family]
    results = run_harness([(stream, wanted) for _, stream, wanted, _ in cases], tmp_path)
    assert len(results) == len(cases)
    for (name, stream, wanted, expected), (status, ended, adler_ok, n_tokens, got) in zip(cases, results):
        if expected is None:
            assert status != 0 and got == b'', (name, status, len(got))
            if family != 'G':
                assert status == dc.STATUS[name], (name, status, dc.STATUS[name])
            continue
        assert status == 0, (name, status)
        assert got == expected, (name, len(got), len(expected))
        whole = wanted >= len(zlib.decompress(stream))
        assert ended == (1 if whole else 0), (name, ended, wanted)
        assert adler_ok == (1 if whole else -1), name
        assert n_tokens <= max(len(expected), 1), name
