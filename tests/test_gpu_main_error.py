"""The 3-D loop's main error over any scalar metrics it records (mtip_set_main_error_ex, k_finish_step's item list) on the MI355X: the
cases of tests/main_error_cases.py -- the four reduction types over the four item sets on both problems, fused and in the reference's
operator order, against the oracle's loop steered by the same main error; the group run; the feedback into
enforce_initial_support; NaN as data; stale and empty metric lists; the C entry's refusals and the bits of the old entry; ccd_diff
on a subset of the orders."""
import pytest

import main_error_cases as MC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'reference_order'])
@pytest.mark.parametrize('item_set', list(MC.ITEM_SETS))
@pytest.mark.parametrize('main_type', MC.TYPES)
@pytest.mark.parametrize('name', ['golden', 'synthetic'])
def test_trajectory_vs_oracle(name, main_type, item_set, fused):
    MC.check_trajectory(name, main_type, item_set, None, fused)


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'reference_order'])
@pytest.mark.parametrize('name,item_set,main_type', MC.EXTRA_CASES, ids=lambda v: str(v))
def test_trajectory_vs_oracle_smaller_support(name, item_set, main_type, fused):
    MC.check_trajectory(name, main_type, item_set, None, fused)


def test_group_trajectory_vs_oracle():
    MC.check_group_trajectory()


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'reference_order'])
def test_main_error_feeds_back(fused):
    MC.check_feedback(fused=fused)


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'reference_order'])
def test_nan_is_data(fused):
    MC.check_nan_main(None, fused)


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'reference_order'])
def test_stale_and_empty_lists(fused):
    MC.check_stale_and_empty(None, fused)


def test_c_entry_refusals():
    MC.check_refusals()


def test_metric_switched_on_late():
    MC.check_metric_switched_on_late()


def test_old_entry_keeps_its_bits():
    MC.check_old_entry_bits()


def test_engine_refusals():
    MC.check_engine_refusals()


def test_ccd_diff_on_order_subset_operator():
    MC.check_ccd_subset_operator()


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'reference_order'])
def test_ccd_diff_on_order_subset_loop(fused):
    MC.check_ccd_subset_loop(None, fused)
