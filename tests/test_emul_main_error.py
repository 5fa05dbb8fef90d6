"""CPU pre-flight of the 3-D loop's main error over any scalar metrics it records (mtip_set_main_error_ex): the unchanged kernel sources on
the CPU emulator through the cases of tests/main_error_cases.py -- every item set and every reduction type once against the oracle's
steered loop, the group run, the feedback into enforce_initial_support, NaN as data, stale and empty metric lists, and what only the
emulator can see: that a refused run launches nothing."""
import os
import subprocess

import pytest

import main_error_cases as MC

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, 'libmtip_emul.so')


@pytest.fixture(scope='session')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EMUL_LIB


@pytest.mark.parametrize('name,main_type,item_set,fused', [('golden', 'min', 'real+II', True), ('golden', 'max', 'real+ccd+rl2', False),
                                                          ('synthetic', 'min', 'real+ccd+rl2', True), ('synthetic', 'mean', 'II', False),
                                                          ('golden', 'prod', 'ranked+real', True),
                                                          ('golden@75', 'min', 'ranked+real', True), ('synthetic@125', 'max', 'real+II', False),
                                                          ('golden@125', 'min', 'real+ccd+rl2', True)],
                         ids=lambda v: str(v))
def test_trajectory_vs_oracle(emul_lib, name, main_type, item_set, fused):
    MC.check_trajectory(name, main_type, item_set, emul_lib, fused)


def test_group_trajectory_vs_oracle(emul_lib):
    MC.check_group_trajectory(lib_path=emul_lib)


def test_main_error_feeds_back(emul_lib):
    MC.check_feedback(lib_path=emul_lib)


def test_nan_is_data(emul_lib):
    MC.check_nan_main(emul_lib)


def test_stale_and_empty_lists(emul_lib):
    MC.check_stale_and_empty(emul_lib)


def test_c_entry_refusals(emul_lib):
    MC.check_refusals(emul_lib)


def test_metric_switched_on_late(emul_lib):
    MC.check_metric_switched_on_late(emul_lib)


def test_old_entry_keeps_its_bits(emul_lib):
    MC.check_old_entry_bits(emul_lib)


def test_engine_refusals(emul_lib):
    MC.check_engine_refusals(emul_lib)


def test_ccd_diff_on_order_subset_operator(emul_lib):
    MC.check_ccd_subset_operator(emul_lib)


def test_ccd_diff_on_order_subset_loop(emul_lib):
    MC.check_ccd_subset_loop(emul_lib)
