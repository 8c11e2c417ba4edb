"""GPU: every entry of the run kernel's tables (tests/h264_run_tables.py) on the device against the oracle, bit-exact on both surfaces."""
import pytest

import frame_cases
import h264_run_tables as T


@pytest.mark.parametrize("run,width", T.RUN_ENTRIES, ids=lambda v: str(v))
@pytest.mark.gpu
def test_run_length_table(mi355, oracle, run, width):
    """four P pictures two macroblock rows high, their rows a designed sequence of macroblock kinds, in one launch of the run kernel with the run length named"""
    T.run_length_entry(mi355, oracle, run, (width,))


@pytest.mark.gpu
def test_run_length_two_widths_in_one_launch(mi355, oracle):
    """pictures 31 and 17 macroblocks wide under one grid at run 15 (11 + 11 + 9): the narrower one's second run is cut short, its third lies beside it"""
    T.run_length_entry(mi355, oracle, *T.MIXED_ENTRY)


@pytest.mark.gpu
def test_run_entry_refuses_a_run_beyond_its_word(mi355):
    """on real descriptors: -1 and untouched surfaces for a run the plan refuses, 0 and the oracle's inter macroblocks for one it takes"""
    T.run_entry_refusals(mi355)


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("name", list(T.B_ENTRIES))
@pytest.mark.gpu
def test_filter_table(mi355, oracle, name, mode):
    """the extreme-sum pictures, the window offsets and the border classes: tiled surfaces (run kernel, fq_two, general code), linear surfaces, second kernel set"""
    T.run_entry(mi355, oracle, name, mode)


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("name", list(T.C_ENTRIES))
@pytest.mark.gpu
def test_weight_table(mi355, oracle, name, mode):
    T.run_entry(mi355, oracle, name, mode)


@pytest.mark.parametrize("name", [n for n in T.C_ENTRIES if n.startswith("explicit")])
@pytest.mark.gpu
def test_weight_table_at_10_bits(mi355, oracle, name):
    """the explicit tables as High 10 pictures: the offsets scaled by the depth"""
    fs, _ = T.entry(oracle, name)
    if not frame_cases.run_case_hbd(mi355, oracle, name, bit_depth=10, fs=fs):
        pytest.skip("oracle/_ref/libref.so not built (no /root/reference)")
