"""CPU: the four tables of tests/hevc_filter_tables.py through the product's kernels under the SIMT emulator — against the oracle (pinned on the reference in
tests/test_hevc_filter_content.py) and the digests recorded from the reference."""
import json

import pytest

import hevc_filter_tables as T
from test_hevc_filter_content import GOLD


@pytest.fixture(scope="module")
def gold():
    return json.load(open(GOLD))


@pytest.mark.parametrize("name", T.LF_CASES)
def test_hevc_filter_tables_deblock_emulated(emu, oracle, gold, name):
    T.check_deblock(emu, oracle, name, gold)


@pytest.mark.parametrize("name", list(T.BS_CASES))
def test_hevc_filter_tables_bs_emulated(emu, oracle, gold, name):
    T.check_bs(emu, oracle, name, gold)


@pytest.mark.parametrize("log2_ctb", list(T.SAO_SIZES))
@pytest.mark.parametrize("bd", T.DEPTHS)
def test_hevc_filter_tables_sao_emulated(emu, oracle, bd, log2_ctb):
    T.check_sao(emu, oracle, bd, log2_ctb)


@pytest.mark.parametrize("name", T.FUSED_CASES)
def test_hevc_filter_tables_fused_emulated(emu, oracle, name):
    T.check_fused(emu, oracle, name)


@pytest.mark.parametrize("form", T.REFUSED_FORMS)
def test_hevc_filter_tables_fused_refusal_emulated(emu, oracle, form):
    T.check_fused_refusal(emu, oracle, form)
