#!/usr/bin/env python3
"""The gfx950 code objects inside libdeepbinner_hip.so, one per source file with kernels: kernel
metadata (registers, spills, scratch, LDS) of every kernel of the library and a census of the forward
kernel's instruction stream.  A kernel's stream is what its ELF symbol covers (disassemble()), so
its count and digest do not depend on which kernels share its code object or on their order.
Used by tests/test_code_object.py and tests/test_code_object_lean.py
(the CPU-box guards on what ships) and by hand: python tools/code_object.py [lib.so]
                                                python tools/code_object.py --same OLD.so NEW.so
                                                python tools/code_object.py --bless [lean]"""
import collections
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = '/opt/rocm/lib/llvm/bin'
BUNDLE = 'hipv4-amdgcn-amd-amdhsa--gfx950'


MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'


def extract(lib, workdir):
    """-> paths of the gfx950 ELF code objects pulled out of lib's .hip_fatbin section, in link order:
    the section is one offload bundle per translation unit with device code, each opened by MAGIC"""
    fat = os.path.join(workdir, 'fatbin')
    subprocess.run([f'{LLVM}/llvm-objcopy', f'--dump-section=.hip_fatbin={fat}', lib, os.path.join(workdir, 'copy.so')],
                   check=True)
    section = open(fat, 'rb').read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), section)]
    out = []
    for i, (a, b) in enumerate(zip(starts, starts[1:] + [len(section)])):
        bundle, co = os.path.join(workdir, f'bundle{i}'), os.path.join(workdir, f'gfx950_{i}.co')
        with open(bundle, 'wb') as f:
            f.write(section[a:b])
        subprocess.run([f'{LLVM}/clang-offload-bundler', '--unbundle', '--type=o', f'--input={bundle}',
                        f'--targets={BUNDLE}', f'--output={co}'], check=True)
        if os.path.getsize(co):
            out.append(co)
    return out


def all_kernel_metadata(lib, workdir):
    """-> {kernel symbol: (code object path, {field: value})} over every code object of lib"""
    found = {}
    for co in extract(lib, workdir):
        for name, m in kernel_metadata(co).items():
            assert name not in found, f'{name} is in two code objects'
            found[name] = (co, m)
    return found


def kernel_metadata(co):
    """-> {kernel symbol: {field: value}} from the AMDGPU metadata note"""
    text = subprocess.run([f'{LLVM}/llvm-readelf', '--notes', co], check=True, capture_output=True,
                          text=True).stdout
    kernels, cur = {}, None
    in_kernels = False
    for line in text.split('\n'):
        if line.strip().startswith('amdhsa.kernels:'):
            in_kernels = True
            continue
        if not in_kernels:
            continue
        if line.startswith('amdhsa.') and not line.startswith('amdhsa.kernels'):
            break
        m = re.match(r'^\s+(- )?\.(\w+):\s+(.*)$', line)
        if not m:
            continue
        dash, key, val = m.groups()
        if dash and re.match(r'^  - ', line):         # a new kernel entry (list item at depth 1)
            cur = {}
            kernels[len(kernels)] = cur
        if cur is not None and re.match(r'^    \.|^  - \.', line):
            cur[key] = val.strip().strip("'")
    return {v['name']: v for v in kernels.values() if 'name' in v}


def symbol_range(co, symbol):
    """-> (address, size) of one function, from the ELF symbol table"""
    text = subprocess.run([f'{LLVM}/llvm-readelf', '-s', '--wide', co], check=True, capture_output=True,
                          text=True).stdout
    for line in text.split('\n'):
        f = line.split()          # Num: Value Size Type Bind Vis Ndx Name
        if len(f) == 8 and f[3] == 'FUNC' and f[7] == symbol:
            return int(f[1], 16), int(f[2], 0)
    raise KeyError(f'{symbol}: no FUNC symbol in {co}')


def disassemble(co, symbol):
    """-> the instruction lines (mnemonic + operands) of one kernel: what lies in [address, address +
    st_size) of its ELF symbol, no more.  (llvm-objdump --disassemble-symbols runs on to the next
    symbol or the end of .text, so the last kernel of a code object came with the section's
    trailing s_nop padding, and its count and digest changed with its neighbours.)  The symbol
    size is the definition: nothing is recognised as padding by its looks.
    Known limit: branch targets are printed relative, but a PC-relative literal that addresses a
    table elsewhere in the code object (s_getpc_b64 + an offset) changes when the kernel moves to
    another unit, although the kernel does not."""
    start, size = symbol_range(co, symbol)
    text = subprocess.run([f'{LLVM}/llvm-objdump', '-d', '--no-show-raw-insn', f'--start-address={start:#x}',
                           f'--stop-address={start + size:#x}', co], check=True, capture_output=True, text=True).stdout
    out = []
    for line in text.split('\n'):
        line = line.split('//')[0].strip()
        if not line or line.endswith(':') or line.startswith(('Disassembly', '/')) or 'file format' in line:
            continue
        out.append(line)
    return out


def census(insts):
    c = collections.Counter()
    for s in insts:
        op = s.split()[0]
        if op.startswith('v_mfma'):
            c['mfma'] += 1
            c['mfma:' + op] += 1
        elif op in ('v_writelane_b32', 'v_readlane_b32'):
            c[op] += 1
        elif op.startswith('v_pk_'):
            c['valu_pk'] += 1
        elif op.startswith('v_'):
            c['valu'] += 1
        elif op.startswith('ds_'):
            c['lds'] += 1
        elif op.startswith('scratch_'):
            c['scratch'] += 1
        elif op.startswith('global_load_lds'):
            c['lds_dma'] += 1
        elif op.startswith(('global_', 'buffer_', 'flat_')):
            c['vmem'] += 1
            if op.startswith('flat_'):
                c['flat'] += 1
        elif op == 's_barrier':
            c['s_barrier'] += 1
        elif op == 's_waitcnt':
            c['s_waitcnt'] += 1
    c['instructions'] = len(insts)
    return dict(c)


# ---------------------------------------------------------------------------------------------
# The hazards the forward kernel keeps BY HAND.  hipcc pads the distance between an MFMA and the first
# instruction that reads its result - for instructions it sees: not for inline asm (the clamped
# packed adds / fmas of the Winograd output transforms, the ds_write_b64 of the edge rows), and its
# own LDS wait counts know nothing of the inline-asm ds_read pipelines.  So the shipped instruction
# stream is checked itself:
#   * a v_mfma_f32_16x16x4_f32 followed by a VALU / LDS / VMEM instruction that READS one of its four
#     result registers needs 10 wait states in between - what hipcc itself pads such a pair to (LLVM's
#     GCNHazardRecognizer, "XDL write VGPR -> VALU / VMEM / LDS read"; the hand-written blocks
#     start with s_nop 7, s_nop 2 = 11); every instruction in between counts one, s_nop N counts N + 1.  (An MFMA reading the result as its accumulator is not
#     subject to this: back-to-back accumulation is what the pipe is for.)
#   * the histogram of the literal `s_waitcnt lgkmcnt(n)` forms - the hand-counted ones are almost
#     all of the n > 0 - is compared with the committed one (tests/golden/code_object.json).
# ---------------------------------------------------------------------------------------------
_REG = re.compile(r'\bv(\d+)\b|\bv\[(\d+):(\d+)\]')


def _vregs(text):
    out = set()
    for m in _REG.finditer(text):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def mfma_read_hazards(insts, need=10):
    """-> [(index, instruction, producing mfma, wait states seen)] of readers that come too early"""
    bad = []
    pending = []                     # (result registers, wait states since, text)
    for i, s in enumerate(insts):
        op = s.split()[0]
        ops = s[len(op):]
        parts = [p.strip() for p in ops.split(',')]
        if op.startswith('v_mfma'):
            reads = _vregs(','.join(parts[1:3]))          # A and B operands (the accumulator is exempt)
            writes = _vregs(parts[0])
        elif op.startswith(('v_', 'ds_', 'global_', 'buffer_', 'flat_', 'scratch_')):
            if op.startswith('v_') and not op.startswith(('v_cmp', 'v_readlane', 'v_readfirstlane')):
                reads, writes = _vregs(','.join(parts[1:])), _vregs(parts[0])
            elif op.startswith(('v_cmp', 'v_readlane', 'v_readfirstlane')):
                reads, writes = _vregs(ops), set()
            elif ('_load' in op or op.startswith('ds_read')) and not op.startswith('global_load_lds'):
                # a load: the first operand is where the data will land (no read; and the register
                # allocator's reuse of an accumulator for it is the compiler's own business)
                reads, writes = _vregs(','.join(parts[1:])), set()
            else:                                         # stores, atomics, LDS-DMA: everything named is read
                reads, writes = _vregs(ops), set()
        else:
            reads, writes = set(), set()
        for regs, since, text in pending:
            if reads & regs and since < need:
                bad.append((i, s, text, since))
        step = 1
        if op == 's_nop':
            step = int(parts[0]) + 1 if parts and parts[0].isdigit() else 1
        pending = [(r, w + step, t) for (r, w, t) in pending if w + step < need and not (writes and writes >= r)]
        if op.startswith('v_mfma'):
            pending.append((writes, 0, s))
    return bad


def lgkm_wait_histogram(insts):
    h = collections.Counter()
    for s in insts:
        m = re.match(r'^s_waitcnt lgkmcnt\((\d+)\)$', s.strip())
        if m:
            h[int(m.group(1))] += 1
    return {str(k): h[k] for k in sorted(h)}


FORWARD = '_ZN3dbh18dbh_forward_kernel'      # dbh::dbh_forward_kernel, whichever code object holds it
LEAN = '_ZN8dbh_lean18dbh_forward_kernel'    # dbh_lean::dbh_forward_kernel (csrc/dbh_lean.hip)
# what --bless writes for which kernel prefix
GOLDEN = {FORWARD: 'code_object.json', LEAN: 'code_object_lean.json'}
META = ('vgpr_count', 'agpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count',
        'private_segment_fixed_size', 'group_segment_fixed_size')


def summary(lib, prefix=FORWARD):
    """everything tests/test_code_object.py looks at, as one dict, for the kernel whose symbol starts
    with `prefix` (the full forward kernel unless told otherwise: LEAN is the lean build's)"""
    with tempfile.TemporaryDirectory() as d:
        md = all_kernel_metadata(lib, d)
        fwd = next(n for n in md if n.startswith(prefix))
        co, meta = md[fwd]
        insts = disassemble(co, fwd)
        c = census(insts)
        return {
            'metadata': {k: meta.get(k) for k in META},
            'census': c,
            'lgkm_waits': lgkm_wait_histogram(insts),
            'mfma_read_hazards': [list(b) for b in mfma_read_hazards(insts)][:20],
        }


def kernels(lib):
    """-> {kernel symbol: (instruction count, hash of the instruction stream, metadata fields)},
    every kernel of the library, each stream cut at its symbol's size (disassemble())"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name, (co, m) in all_kernel_metadata(lib, d).items():
            insts = disassemble(co, name)
            digest = hashlib.sha256('\n'.join(insts).encode()).hexdigest()[:16]
            out[name] = (len(insts), digest, {k: m.get(k) for k in META + ('kernarg_segment_size',)})
    return out


def same(old_lib, new_lib):
    """the kernels of two builds side by side, for a change that must not alter the compiled code -
    a kernel moved to another source file or given other neighbours included (disassemble() has the
    one known limit): -> (report lines, number of kernels present on both sides that differ)"""
    old, new = kernels(old_lib), kernels(new_lib)
    lines, differ = [], 0
    for name in sorted(set(old) & set(new)):
        (n0, h0, m0), (n1, h1, m1) = old[name], new[name]
        ok = (n0, h0, m0) == (n1, h1, m1)
        differ += not ok
        meta = ' '.join(f'{k}={m0[k]}' if m0[k] == m1[k] else f'{k}={m0[k]}->{m1[k]}' for k in m0)
        lines.append(f"{'same' if ok else 'DIFFERS'} {name}\n     instructions {n0 if n0 == n1 else f'{n0}->{n1}'}"
                     f" stream {h0 if h0 == h1 else f'{h0}->{h1}'}\n     {meta}")
    for side, only in (('old', set(old) - set(new)), ('new', set(new) - set(old))):
        for name in sorted(only):
            n, h, _ = (old if side == 'old' else new)[name]
            lines.append(f'only in {side}: {name}\n     instructions {n} stream {h}')
    return lines, differ


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--same':
        # python tools/code_object.py --same OLD.so NEW.so: exit status 1 if a kernel of both differs
        lines, differ = same(sys.argv[2], sys.argv[3])
        print('\n'.join(lines))
        print(f'{differ} kernel(s) differ')
        sys.exit(1 if differ else 0)
    if len(sys.argv) > 1 and sys.argv[1] == '--bless':
        # record what the built library carries (tests/golden/code_object.json): run after every
        # deliberate change of the forward kernel, and read the diff.  --bless PREFIX (or `lean`)
        # does the same for another build of it: `--bless lean` writes code_object_lean.json
        lib = os.path.join(os.path.dirname(__file__), '..', 'deepbinner_amd', 'libdeepbinner_hip.so')
        prefix = FORWARD if len(sys.argv) < 3 else LEAN if sys.argv[2] == 'lean' else sys.argv[2]
        if prefix not in GOLDEN:
            sys.exit(f'--bless: no golden file for kernel prefix {prefix!r} (known: {sorted(GOLDEN)})')
        s = summary(lib, prefix)
        keep = {'mfma_static': s['census']['mfma'], 'lds_dma': s['census'].get('lds_dma', 0),
                's_barrier': s['census'].get('s_barrier', 0), 'lgkm_waits': s['lgkm_waits'],
                'vgpr_count': int(s['metadata']['vgpr_count']), 'sgpr_spill_count': int(s['metadata']['sgpr_spill_count'])}
        path = os.path.join(os.path.dirname(__file__), '..', 'tests', 'golden', GOLDEN[prefix])
        json.dump(keep, open(path, 'w'), indent=1, sort_keys=True)
        print(json.dumps(keep, indent=1, sort_keys=True))
        return
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), '..', 'deepbinner_amd',
                                                             'libdeepbinner_hip.so')
    with tempfile.TemporaryDirectory() as d:
        md = all_kernel_metadata(lib, d)
        out = {}
        for name, (_, m) in md.items():
            keep = {k: m.get(k) for k in ('vgpr_count', 'agpr_count', 'sgpr_count', 'vgpr_spill_count',
                                          'sgpr_spill_count', 'private_segment_fixed_size',
                                          'group_segment_fixed_size', 'max_flat_workgroup_size')}
            out[name] = keep
        fwd = next(n for n in md if n.startswith(FORWARD))
        out['forward_census'] = census(disassemble(md[fwd][0], fwd))
        print(json.dumps(out, indent=1))


if __name__ == '__main__':
    main()
