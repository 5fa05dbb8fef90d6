"""Converged-ER-state fixture for the projection's well-posed comparisons (parity_cases.check_projection_converged_er_state):
the 16 x L4 golden problem through the product's loop on the CPU emulation of the kernels (tests/emul) with the shadow harness
of parity_cases, schedule shadow_golden_schedule (2 x (60 HIO, SW, 40 ER), SW, 40 ER), one restart from the fixture's rho0;
the densities before and after the last step are kept:

  rho_prev, rho     (16, 8, 16) complex: restart 0 before / after step 239 (ER, ft_stab)

Written to tests/golden/converged_er_N16_L4.npz.  usage: python tests/golden/make_converged_er_fixture.py"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    np.seterr(all='ignore')
    import parity_cases as PC
    from oracle import mtip as OM
    from xframe_amd.fxs import reconstruct as R
    emul = os.path.join(ROOT, 'tests', 'emul')
    subprocess.run(['make', '-C', emul, '-j6'], check=True, capture_output=True)
    g = np.load(os.path.join(HERE, 'mtip_N16_L4.npz'))
    opt, data = PC.shadow_golden_schedule(g)
    total = PC._schedule_length(opt)
    R.MTIP.preinit(opt, data)
    m = R.MTIP(n_restarts=1, initial_densities=[g['rho0']], lib_path=os.path.join(emul, 'libmtip_emul.so'))
    m.generate_phasing_loop()
    sh = PC._Shadow(m.engine, OM.MTIP(opt, data), total, total, True)
    m.phasing_loop()
    m.engine.close()
    step, _, _, _, rho_prev, rho = sh.states[-1]
    assert step == total - 1
    np.savez_compressed(os.path.join(HERE, 'converged_er_N16_L4.npz'), rho_prev=rho_prev, rho=rho)


if __name__ == '__main__':
    main()
