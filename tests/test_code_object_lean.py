"""The CPU-box guard of tests/test_code_object.py on the LEAN build of the forward kernel
(dbh_lean::dbh_forward_kernel, csrc/dbh_lean.hip): the kernel production launches run.  It is the
same source as the full kernel with the debug stages folded away, so it does the same matrix work
(static MFMA and LDS-DMA counts equal to the full kernel's golden) and has the same hand-counted
waits in its source; what the compiler derives around them - spilled scalars, the histogram of the
literal `s_waitcnt lgkmcnt(n)` sites - is pinned in a golden of its own
(tests/golden/code_object_lean.json, `python tools/code_object.py --bless lean`)."""
import json
import os
import sys
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import code_object                                           # noqa: E402

from test_code_object import layout_constants               # noqa: E402

LIB = os.path.join(REPO, 'deepbinner_amd', 'libdeepbinner_hip.so')
GOLD_FULL = os.path.join(REPO, 'tests', 'golden', 'code_object.json')
GOLD_LEAN = os.path.join(REPO, 'tests', 'golden', 'code_object_lean.json')

pytestmark = pytest.mark.skipif(not os.path.exists(code_object.LLVM + '/llvm-objdump'),
                                reason='no ROCm LLVM tools here')


@pytest.fixture(scope='module')
def lean():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return code_object.summary(LIB, code_object.LEAN)


def test_lean_kernel_registers_and_memory(lean):
    md = lean['metadata']
    assert int(md['vgpr_count']) <= 256 and int(md['agpr_count']) == 0
    assert int(md['vgpr_spill_count']) == 0, 'the lean forward kernel spills vector registers'
    assert int(md['private_segment_fixed_size']) == 0, 'the lean forward kernel uses scratch memory'
    lds_floats, _ = layout_constants()
    assert int(md['group_segment_fixed_size']) == 4 * lds_floats <= 160 * 1024
    assert lean['census'].get('scratch', 0) == 0


def test_lean_kernel_does_the_full_kernels_matrix_work(lean):
    c = lean['census']
    mfma_ops = [k for k in c if k.startswith('mfma:')]
    assert mfma_ops == ['mfma:v_mfma_f32_16x16x4_f32'], mfma_ops          # exact fp32: nothing else
    full = json.load(open(GOLD_FULL))
    # same source, same matrix work: the FULL kernel's golden, not one of its own
    assert c['mfma'] == full['mfma_static'] == 2490
    assert c.get('lds_dma', 0) == full['lds_dma'] == 171


def test_lean_kernel_hazards_and_derived_waits(lean):
    assert lean['mfma_read_hazards'] == [], lean['mfma_read_hazards'][:5]
    gold = json.load(open(GOLD_LEAN))
    assert int(lean['metadata']['sgpr_spill_count']) == gold['sgpr_spill_count']
    assert lean['lgkm_waits'] == gold['lgkm_waits'], (
        'the LDS wait counts of the lean forward kernel changed - if that was meant: '
        'python tools/code_object.py --bless lean, and read the diff')


def test_lean_kernel_is_its_own_symbol_and_ends_where_it_ends(lean):
    with tempfile.TemporaryDirectory() as d:
        md = code_object.all_kernel_metadata(LIB, d)
        names = [n for n in md if n.startswith(code_object.LEAN)]
        assert len(names) == 1, names
        assert code_object.disassemble(md[names[0]][0], names[0])[-1] == 's_endpgm'
    # the default of summary() is still the full kernel (tests/test_code_object.py calls it so)
    assert code_object.FORWARD != code_object.LEAN and code_object.GOLDEN[code_object.FORWARD] == 'code_object.json'
