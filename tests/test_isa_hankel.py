"""Static check of the Hankel tile kernels the benchmark runs, k_hankel_tile<1|2, false|true>, on the gfx950 listing
(scripts/isa_census.py), in the manner of tests/test_isa_chain.py.

The conditions are the description in xframe_amd/csrc/k_hankel.hip: a stage requests its W fragments and its panel in 16-byte
loads, deposits the panel once, meets at one barrier and then multiplies with A from registers and B from LDS, the next stage's
operands in flight.  The k-steps of a stage are unrolled (the A values live in registers, which cannot be indexed at run time) and
the stage loop is written out for its two register sets, so "the loop that holds the MFMAs" is, behind each barrier, the stretch
from the first to the last MFMA in front of the next barrier: it has no global or flat access, no wait for one, no barrier and no
EXEC-mask region.  They name what the kernel should contain, not tuned counts.  No GPU needed: hipcc cross-compiles.  One
compilation is shared by the tests of this file."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import isa_census  # noqa: E402

SRC = os.path.join(ROOT, 'xframe_amd', 'csrc', 'k_hankel.hip')
KINDS = {'ct1': 'k_hankel_tile<1, false>', 'ct1_sub': 'k_hankel_tile<1, true>',
         'ct2': 'k_hankel_tile<2, false>', 'ct2_sub': 'k_hankel_tile<2, true>'}
MAX_VGPRS = 128


def _hipcc():
    hipcc, _ = isa_census.makefile_flags()
    return hipcc if os.path.exists(hipcc) else shutil.which('hipcc')


def _body(text, symbol):
    """(mnemonic, operands) of the kernel's instructions in listing order, and the set of indices that are back-branch targets"""
    lines = text.splitlines()
    start = next(i for i, s in enumerate(lines) if s.startswith(symbol + ':'))
    body, labels = [], {}
    for s in lines[start + 1:]:
        if s.startswith('.Lfunc_end'):
            break
        lm = isa_census._LABEL.match(s)
        if lm:
            labels[lm.group(1)] = len(body)
            continue
        im = isa_census._INSTR.match(s)
        if im and not im.group(1).startswith('.') and isa_census.classify(im.group(1), im.group(2) or '') is not None:
            body.append((im.group(1), im.group(2) or ''))
    return body, labels


@pytest.fixture(scope='module')
def kernels():
    if _hipcc() is None:
        pytest.skip('hipcc not found')
    text = isa_census.compile_listing(SRC)
    found = isa_census.census_of_listing(text)
    out = {}
    for kind, name in KINDS.items():
        ks = [k for k in found if name in k.name]
        assert len(ks) == 1, (kind, [k.name for k in found])
        out[kind] = (ks[0],) + _body(text, ks[0].symbol)
    return out


def _mfma_stretches(body):
    """per stretch of the listing between two barriers (or the kernel's ends) that holds MFMAs: (first, last) index of its MFMAs"""
    cuts = [-1] + [i for i, (m, _) in enumerate(body) if m == 's_barrier'] + [len(body)]
    out = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        at = [i for i in range(lo + 1, hi) if body[i][0].startswith('v_mfma')]
        if at:
            out.append((at[0], at[-1]))
    return out


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_mfma_stretch_is_registers_and_lds(kernels, kind):
    k, body, labels = kernels[kind]
    assert all(m == 'v_mfma_f64_16x16x4_f64' for m, _ in body if m.startswith('v_mfma'))
    stretches = _mfma_stretches(body)
    assert stretches and body[:stretches[0][0]].count(('s_barrier', '')) >= 1, 'no MFMA in front of the first barrier'
    for first, last in stretches:
        stretch = body[first:last + 1]
        mfma = sum(1 for m, _ in stretch if m.startswith('v_mfma'))
        lds = sum(1 for m, _ in stretch if m.startswith('ds_read'))
        print('%s: %d instructions from the first to the last of %d MFMAs, %d LDS reads' % (kind, len(stretch), mfma, lds))
        assert lds > 0, 'the B fragments come from LDS'
        for m, ops in stretch:
            assert not m.startswith(('global_', 'flat_', 'buffer_', 'scratch_')), (m, ops)
            assert not (m.startswith('s_waitcnt') and 'vmcnt' in ops), 'a wait for global memory between the MFMAs'
            assert 'saveexec' not in m and not re.match(r'exec(_lo|_hi)?\b', ops), ('EXEC is written between the MFMAs', m, ops)
        # the stretch is one stage's k-steps: no loop closes inside it
        for i in range(first, last + 1):
            m, ops = body[i]
            if m.startswith('s_cbranch') or m == 's_branch':
                target = ops.split(',')[-1].strip()
                assert not (target in labels and first < labels[target] <= i), 'a loop inside the MFMA stretch'


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_operand_loads_are_16_bytes(kernels, kind):
    """W fragments and panel pairs arrive in global_load_dwordx4; only the mask byte (and the tile record, a scalar load) is
    narrower"""
    k, body, _ = kernels[kind]
    loads = [m for m, _ in body if m.startswith(('global_load', 'flat_load', 'buffer_load'))]
    narrow = [m for m in loads if m != 'global_load_dwordx4']
    print('%s: %d loads, narrower: %s' % (kind, len(loads), narrow))
    assert loads.count('global_load_dwordx4') > 0
    assert all(m == 'global_load_ubyte' for m in narrow) and len(narrow) <= (1 if kind.endswith('sub') else 0), narrow


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_one_barrier_per_stage_and_registers(kernels, kind):
    """one barrier per stage, behind its deposit (the stage loop is written out for two stages); no scratch, at most 128 VGPRs"""
    k, body, _ = kernels[kind]
    barriers = sum(1 for m, _ in body if m == 's_barrier')
    print('%s: %d s_barrier, VGPRs %d, AGPRs %d, ScratchSize %d' % (kind, barriers, k.vgprs, k.agprs, k.scratch))
    assert 1 <= barriers <= 2
    assert k.scratch == 0
    assert 0 < k.vgprs <= MAX_VGPRS
