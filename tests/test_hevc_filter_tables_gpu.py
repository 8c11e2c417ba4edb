"""GPU: the four tables of tests/hevc_filter_tables.py through the product on an MI355X — against the oracle (pinned on the reference in
tests/test_hevc_filter_content.py) and the digests recorded from the reference.  The refusals are ones the API defines (a job form the fused entry point does
not take): each runs once, nothing faults."""
import json

import pytest

import hevc_filter_tables as T
from test_hevc_filter_content import GOLD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return json.load(open(GOLD))


@pytest.mark.parametrize("name", T.LF_CASES)
def test_hevc_filter_tables_deblock_gpu(mi355, oracle, gold, name):
    T.check_deblock(mi355, oracle, name, gold)


@pytest.mark.parametrize("name", list(T.BS_CASES))
def test_hevc_filter_tables_bs_gpu(mi355, oracle, gold, name):
    T.check_bs(mi355, oracle, name, gold)


@pytest.mark.parametrize("log2_ctb", list(T.SAO_SIZES))
@pytest.mark.parametrize("bd", T.DEPTHS)
def test_hevc_filter_tables_sao_gpu(mi355, oracle, bd, log2_ctb):
    T.check_sao(mi355, oracle, bd, log2_ctb)


@pytest.mark.parametrize("name", T.FUSED_CASES)
def test_hevc_filter_tables_fused_gpu(mi355, oracle, name):
    T.check_fused(mi355, oracle, name)


@pytest.mark.parametrize("form", T.REFUSED_FORMS)
def test_hevc_filter_tables_fused_refusal_gpu(mi355, oracle, form):
    T.check_fused_refusal(mi355, oracle, form)
