"""GPU: SWS_FAST_BILINEAR contexts (mi355_sws_create_fast_bilinear) of the device swscale path: the instances of k_sws_fbl_generic / k_sws_fbl_planar
(sws_fastbl.hip).

Every row of tests/sws_fastbl.py on the contexts committed in tests/golden/sws_fastbl_contexts.npz: a guarded four-frame Tier-2 batch — the source
planes on 16-byte multiples with a wider stride, at stride = width + 1, at stride == width with one byte behind the last line, and that class again at
an odd address; noise everywhere around the pictures — is byte for byte the reference's own sws_scale() of the same buffers as the fixture holds it
(sha1 per frame, frame 0 of the first rows in full); one Tier-1 call per row; without the fixture, every row whose increments never reach x = srcW
against the existing creator's context on the equivalent two-tap banks; the line entries against the numpy restatement; the refusals and the twin rule on
the real library.  Nothing but that fixture is read: neither the reference's sources nor a library built from them."""
import pytest

import sws_fastbl as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", F.NAMES)
def test_fast_bilinear_batched_on_the_device(mi355, name):
    p = F.check_batch(mi355.lib, name)
    assert p["fast"] == 1 and p["kernel"].startswith(("generic_", "planar_")) and p["hstage"] == 1, (name, p)


@pytest.mark.parametrize("name", F.NAMES)
def test_fast_bilinear_tier1(mi355, name):
    # (the second picture reuses the context's device buffers)
    F.check_tier1(mi355.lib, name)


@pytest.mark.parametrize("name", [n for n in F.NAMES if F.qualifies(n)])
def test_fast_bilinear_equals_the_existing_creator_on_two_tap_banks(mi355, name):
    F.check_cross(mi355.lib, name)


def test_fast_bilinear_line_entries_on_the_device(mi355):
    assert F.check_line_entries(mi355.lib) == 5 * 5 * 2


def test_fast_bilinear_refusals_and_twin_rule_on_the_device(mi355):
    lib = mi355.lib
    for what, e in F.refusal_cases():
        assert not F.create(lib, e), what
    for n in F.NAMES:
        e = F.stored_entry(n)
        p, t = F.plan(lib, e), F.twin_plan(lib, e)
        assert p is not None and t is not None, n
        assert all(p[k] == t[k] for k in F.TWIN_KEYS), (n, p, t)
        assert (p["fast"], p["lum_inc"], p["chr_inc"], p["layout"], p["alpha"]) == (1, e.lum_inc, e.chr_inc, 0, 0), (n, p)
        assert (t["fast"], t["lum_inc"], t["chr_inc"]) == (0, 0, 0), n
