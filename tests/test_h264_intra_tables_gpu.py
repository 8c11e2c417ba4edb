"""GPU: every entry of the intra tables (tests/h264_intra_tables.py) on the device against the frame-level oracle, bit-exact on both surfaces."""
import pytest

import h264_intra_tables as T


@pytest.mark.parametrize("form", T.FORMS8)
@pytest.mark.parametrize("name", T.ENTRIES)
@pytest.mark.gpu
def test_intra_table(mi355, oracle, name, form):
    """first kernel set: linear and tiled surfaces, a launch per level and the single launch (which the plan must report); second kernel set at 8 bit"""
    assert T.run_entry(mi355, oracle, name, form)


@pytest.mark.parametrize("form", T.FORMS_HBD)
@pytest.mark.parametrize("name", T.ENTRIES)
@pytest.mark.gpu
def test_intra_table_above_8_bits(mi355, oracle, name, form):
    """second kernel set at 9 and 10 bit 4:2:0 and 10 bit 4:2:2, the carriers built at that depth"""
    if not T.run_entry(mi355, oracle, name, form):
        pytest.skip("oracle/_ref/libref.so not built (no /root/reference)")
