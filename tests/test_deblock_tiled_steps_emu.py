"""CPU: the tiled loop filter's step addressing (ring slots, the columns of the horizontal edges, the strengths' lanes, the hand-down
between bands) on the table of deblock_step_cases under the SIMT emulator, both tiled forms against the oracle; and what the table's
content reaches, asserted from the oracle's pictures alone, so that a table that stops reaching an edge class fails instead of passing empty."""
import pytest

import deblock_step_cases as S


def test_table_reaches_every_edge_class():
    ec, cen = S.table_census()
    print(sorted(ec.items()))
    for k in S.CLASSES:
        assert ec.get(k, 0) > 0, (k, ec)
    # strengths 0 .. 4 in both directions, on macroblock edges (4: intra) and inside (3: intra), P and B pictures, several slices
    for d in (0, 1):
        for k in ["bs%d_mb_%d" % (b, d) for b in (0, 1, 2, 4)] + ["bs%d_in_%d" % (b, d) for b in (0, 1, 2, 3)]:
            assert cen.get(k, 0) > 0, (k, cen)
    for k in ("b_picture", "dct8", "cross_slice_edge", "pcm_inter_edge", "seg_luma4_changed", "seg_luma123_changed", "seg_chroma_changed", "seg_luma123_kept"):
        assert cen.get(k, 0) > 0, (k, cen)


@pytest.mark.parametrize("w,h", S.SHAPES, ids=["%dx%d" % s for s in S.SHAPES])
def test_tiled_forms_step_table_emulated(emu, w, h):
    S.run_shape(emu, w, h)
