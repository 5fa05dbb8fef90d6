"""Record the bits of the Hankel tile kernel for tests/hankel_onepass_cases.py (check_bits) into tests/golden/hankel_bits.npz.

The one-pass kernel must give every accumulator the MFMA sequence of the workgroup-tiled, chunked kernel it replaced, so its
results are compared bit for bit with those of the commit in front of it.  Run this with THAT commit's libraries, once per kind:

    python tests/golden/make_golden_hankel_bits.py emul PATH/libmtip_emul.so COMMIT       (CPU emulator)
    python tests/golden/make_golden_hankel_bits.py gpu  PATH/libmtip_hip.so  COMMIT       (MI355X)

Each run records the forward, the inverse and the difference transform of the seeded problem under KIND_fwd, KIND_inv, KIND_diff
and keeps what the file already holds of the other kind; both runs must name the same commit (stored as parent_commit).  The
recorded library must itself give the same bits at every tile width (asserted)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import hankel_onepass_cases as OC  # noqa: E402


def main(kind, lib_path, commit):
    assert kind in ('emul', 'gpu'), kind
    by_width = {}
    for ct in (1, 2, 3, 5):
        os.environ['MTIP_HANKEL_CT'] = str(ct)
        by_width[ct] = OC.bits_results(os.path.abspath(lib_path), ct)
    print(OC.check_bits_within_bound(by_width[1]))
    for key in OC.BITS_KEYS:
        for ct in (2, 3, 5):
            assert np.array_equal(by_width[ct][key], by_width[1][key]), (key, ct)
    held = dict(np.load(OC.GOLDEN)) if os.path.exists(OC.GOLDEN) else {}
    if 'parent_commit' in held:
        assert str(held['parent_commit']) == commit, (str(held['parent_commit']), commit)
    held['parent_commit'] = np.array(commit)
    for key in OC.BITS_KEYS:
        held['%s_%s' % (kind, key)] = by_width[1][key]
    np.savez(OC.GOLDEN, **held)
    print('wrote', OC.GOLDEN, sorted(held))


if __name__ == '__main__':
    main(*sys.argv[1:4])
