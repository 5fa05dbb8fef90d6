"""Record the bits of the chained inverse -> forward SHT kernels for tests/chain_diet_cases.py into tests/golden/chain_bits.npz.

The leaner L = 32 instantiation of k_sht_chain must give every output the operations, in the order, of the kernel it replaced,
so its results are compared bit for bit with those of the commit in front of it.  Run this with THAT commit's libraries, once per
kind:

    python tests/golden/make_golden_chain_bits.py emul PATH/libmtip_emul.so COMMIT       (CPU emulator)
    python tests/golden/make_golden_chain_bits.py gpu  PATH/libmtip_hip.so  COMMIT       (MI355X)

Each run records the cases of chain_diet_cases (transforms at the three shapes, fused steps at the L = 32 shape) under KIND_* and
keeps what the file already holds of the other kind; both runs must name the same commit (stored as parent_commit).  An optional
fourth argument names the file to write (default: tests/golden/chain_bits.npz)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import chain_diet_cases as DC  # noqa: E402


def main(kind, lib_path, commit, out=None):
    assert kind in ('emul', 'gpu'), kind
    out = out or DC.GOLDEN
    lib_path = os.path.abspath(lib_path)
    src = out if os.path.exists(out) else DC.GOLDEN
    held = dict(np.load(src)) if os.path.exists(src) else {}
    if 'parent_commit' in held:
        assert str(held['parent_commit']) == commit, (str(held['parent_commit']), commit)
    held['parent_commit'] = np.array(commit)
    for name in DC.CASES:
        DC.record(DC.transform_results(name, lib_path), kind, held)
    DC.record(DC.steps_results(lib_path), kind, held)
    np.savez(out, **held)
    print('wrote', out, os.path.getsize(out), 'bytes', len(held), 'entries')


if __name__ == '__main__':
    main(*sys.argv[1:5])
