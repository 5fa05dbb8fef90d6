"""Instruction census of the barrier loops of a HIP translation unit, from the gfx950 assembly the compiler emits.

The Jacobi round of k_rproj (and the chained SHT steps) are bound by the NUMBER of instructions a wave issues between two
barriers, so that number -- and what it is made of -- is the quantity to watch.  This tool compiles one .hip file to assembly
with the flags of xframe_amd/csrc/Makefile (device side only), finds the loops of every kernel by label and back-branch and
prints, for every loop that holds exactly one s_barrier, the instruction count by class, next to the kernel's register and
scratch figures.

usage: python scripts/isa_census.py xframe_amd/csrc/k_projr.hip [--kernel REGEX] [--all-loops] [--asm FILE] [--keep FILE]
  --kernel REGEX   only kernels whose demangled name matches
  --all-loops      every loop, whatever its number of barriers
  --asm FILE       read this listing instead of compiling
  --keep FILE      keep the listing the compiler wrote

As a module: census(path_to_hip) or census_of_listing(text) return a list of KernelCensus."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from collections import Counter, namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'xframe_amd', 'csrc')

CLASSES = ('fp64', 'lds', 'dpp', 'cndmask', 'readlane', 'writelane', 'v_mov', 'saveexec', 'scalar', 'waitcnt', 'valu_other',
           'memory')
Loop = namedtuple('Loop', 'label first_line last_line barriers total counts detail')
KernelCensus = namedtuple('KernelCensus', 'symbol name vgprs agprs sgprs scratch loops')


def makefile_flags():
    """CXXFLAGS of the library's Makefile with its variables expanded: (hipcc, [flags])."""
    text = open(os.path.join(CSRC, 'Makefile')).read()
    var = {}
    for m in re.finditer(r'^(\w+)\s*\??=\s*(.*)$', text, re.M):
        var[m.group(1)] = m.group(2).strip()
    flags = re.sub(r'\$\((\w+)\)', lambda m: var.get(m.group(1), ''), var['CXXFLAGS'])
    hipcc = os.environ.get('HIPCC') or var.get('HIPCC', 'hipcc')
    if not os.path.exists(hipcc):
        hipcc = shutil.which('hipcc') or hipcc
    return hipcc, flags.split()


def compile_listing(src, keep=None):
    hipcc, flags = makefile_flags()
    out = keep or tempfile.mktemp(suffix='.s')
    try:
        r = subprocess.run([hipcc] + flags + ['--cuda-device-only', '-S', os.path.abspath(src), '-o', out],
                           cwd=os.path.dirname(os.path.abspath(src)), capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError('hipcc failed:\n' + r.stderr[-4000:])
        return open(out).read()
    finally:
        if keep is None and os.path.exists(out):
            os.unlink(out)


def classify(mnemonic, operands):
    """Class of one instruction, one of CLASSES (None for what is no instruction)."""
    m = mnemonic
    if m.startswith('ds_'):
        return 'lds'
    if m.startswith(('global_', 'flat_', 'scratch_', 'buffer_', 's_load_', 's_buffer_load', 's_scratch_load')):
        return 'memory'
    if m.startswith('s_'):
        if 'saveexec' in m:
            return 'saveexec'
        if m.startswith('s_waitcnt'):
            return 'waitcnt'
        return 'scalar'
    if m.startswith('v_'):
        if m.startswith('v_readlane') or m.startswith('v_readfirstlane'):
            return 'readlane'
        if m.startswith('v_writelane'):
            return 'writelane'
        if m.endswith('_dpp') or re.search(r'\b(quad_perm|row_shl|row_shr|row_ror|row_mirror|row_half_mirror|row_bcast|row_newbcast|'
                                            r'wave_shl|wave_shr|wave_rol|wave_ror)\b', operands):
            return 'dpp'
        if m.startswith('v_cndmask'):
            return 'cndmask'
        if '_f64' in m:
            return 'fp64'
        if re.match(r'v_mov_b(32|64)', m) or m.startswith('v_accvgpr_'):
            return 'v_mov'
        return 'valu_other'
    return None


_INSTR = re.compile(r'^\s+([a-z][a-z0-9_]+)(?:\s+(.*?))?\s*(?://.*|;.*)?$')
_LABEL = re.compile(r'^([.\w$]+):')


def demangle(symbols):
    tool = shutil.which('llvm-cxxfilt') or shutil.which('c++filt')
    for cand in ('/opt/rocm/llvm/bin/llvm-cxxfilt', '/opt/rocm/lib/llvm/bin/llvm-cxxfilt'):
        if tool is None and os.path.exists(cand):
            tool = cand
    if tool is None or not symbols:
        return {s: s for s in symbols}
    r = subprocess.run([tool], input='\n'.join(symbols), capture_output=True, text=True)
    names = r.stdout.splitlines()
    return dict(zip(symbols, names)) if len(names) == len(symbols) else {s: s for s in symbols}


def census_of_listing(text):
    lines = text.splitlines()
    kernels = set(re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', text, re.M))
    out = []
    i = 0
    while i < len(lines):
        m = _LABEL.match(lines[i])
        if not (m and m.group(1) in kernels):
            i += 1
            continue
        sym = m.group(1)
        end = i + 1
        while end < len(lines) and not lines[end].startswith('.Lfunc_end'):
            end += 1
        # instructions and labels of the body
        body = []                                         # (line number, mnemonic, operands)
        labels = {}                                       # label -> index into body of the first instruction behind it
        for ln in range(i + 1, end):
            s = lines[ln]
            lm = _LABEL.match(s)
            if lm:
                labels[lm.group(1)] = len(body)
                continue
            im = _INSTR.match(s)
            if im and not im.group(1).startswith('.') and classify(im.group(1), im.group(2) or '') is not None:
                body.append((ln + 1, im.group(1), im.group(2) or ''))
        loops = []
        for idx, (ln, mn, ops) in enumerate(body):
            if not (mn.startswith('s_cbranch') or mn == 's_branch'):
                continue
            target = ops.split(',')[-1].strip()
            if target in labels and labels[target] <= idx:                # back-branch: a loop from the label to here
                span = body[labels[target]:idx + 1]
                counts = Counter(classify(a, b) for _, a, b in span)
                detail = Counter()
                for _, a, b in span:
                    if a.startswith('scratch_'):
                        detail['scratch'] += 1
                    if a.startswith('flat_'):
                        detail['flat'] += 1
                    if re.match(r'v_mov_b64', a) and classify(a, b) == 'v_mov':
                        detail['v_mov_b64'] += 1
                    if a.startswith('s_nop'):
                        detail['s_nop'] += 1
                    if a.startswith('s_cbranch') or a == 's_branch':
                        detail['branch'] += 1
                    if a.startswith(('s_memtime', 's_memrealtime')):       # clock64(): a diagnostic instance with timers
                        detail['clock'] += 1
                    if a.startswith('v_mfma'):
                        detail['mfma'] += 1
                    if a == 's_endpgm':                                     # no loop: a block placed behind the kernel's end that jumps back
                        detail['endpgm'] += 1
                    if a.startswith('ds_read_b128'):
                        detail['ds_read_b128'] += 1
                    if a.startswith('ds_write'):
                        detail['lds_store'] += 1
                    if a.startswith('global_'):
                        detail['global'] += 1
                    if a.startswith('global_load'):
                        detail['global_load'] += 1
                    if a.startswith('s_waitcnt') and 'vmcnt(' in b:
                        detail['vmcnt'] += 1
                        if 'vmcnt(0)' in b:
                            detail['vmcnt0'] += 1
                barriers = sum(1 for _, a, _b in span if a == 's_barrier')
                loops.append(Loop(target, span[0][0], ln, barriers, len(span), counts, detail))
        # the figures the compiler prints behind the kernel
        meta = '\n'.join(lines[end:end + 400])
        mm = re.search(r'\.end_amdhsa_kernel(.*?)(?:\.Lfunc_begin|\Z)', meta, re.S)
        meta = mm.group(1) if mm else meta

        def fig(key):
            g = re.search(r';\s*' + key + r':\s*(\d+)', meta)
            return int(g.group(1)) if g else -1
        out.append([sym, fig('NumVgprs'), fig('NumAgprs'), fig('TotalNumSgprs'), fig('ScratchSize'), loops])
        i = end
    names = demangle([k[0] for k in out])
    return [KernelCensus(k[0], names[k[0]], k[1], k[2], k[3], k[4], k[5]) for k in out]


def census(src):
    return census_of_listing(compile_listing(src))


def format_census(kernels, all_loops=False, pattern=None):
    rows = []
    head = '%-10s %11s %5s | ' % ('loop', 'lines', 'total') + ' '.join('%9s' % c for c in CLASSES) + ' | notes'
    for k in kernels:
        if pattern and not re.search(pattern, k.name):
            continue
        rows.append('%s' % k.name)
        rows.append('  VGPRs %d  AGPRs %d  SGPRs %d  ScratchSize %d' % (k.vgprs, k.agprs, k.sgprs, k.scratch))
        shown = [lp for lp in k.loops if all_loops or lp.barriers == 1]
        if not shown:
            rows.append('  (no loop with exactly one s_barrier)')
            continue
        rows.append('  ' + head)
        for lp in sorted(shown, key=lambda x: x.first_line):
            notes = ', '.join('%s %d' % (n, c) for n, c in sorted(lp.detail.items()))
            if all_loops:
                notes = ('barriers %d' % lp.barriers) + (', ' + notes if notes else '')
            rows.append('  %-10s %5d-%-5d %5d | ' % (lp.label, lp.first_line, lp.last_line, lp.total) +
                        ' '.join('%9d' % lp.counts.get(c, 0) for c in CLASSES) + ' | ' + notes)
    return '\n'.join(rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('source')
    ap.add_argument('--kernel')
    ap.add_argument('--all-loops', action='store_true')
    ap.add_argument('--asm')
    ap.add_argument('--keep')
    a = ap.parse_args()
    text = open(a.asm).read() if a.asm else compile_listing(a.source, a.keep)
    print('# %s: loops with %s, instructions by class' % (os.path.relpath(os.path.abspath(a.source), ROOT),
                                                         'any number of barriers' if a.all_loops else 'exactly one s_barrier'))
    print(format_census(census_of_listing(text), a.all_loops, a.kernel))


if __name__ == '__main__':
    sys.exit(main())
