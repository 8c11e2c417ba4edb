"""GPU: planar RGB (gbrp) destinations (mi355_sws_create_gbrp) of the device swscale path: the instances of k_sws_gbrp (sws_gbrp.hip).

Every row of tests/sws_gbrp.py on the contexts committed in tests/golden/sws_gbrp_contexts.npz: a guarded four-frame Tier-2 batch — the source planes
on 16-byte multiples, on 4-byte multiples, at the source's least aligned position and at another stride 8 bytes in; full-range noise in two frames,
nominal-range noise in two; noise everywhere around the pictures; the destination planes aligned in frame 0 and unaligned in the others — is byte for
byte the reference's own sws_scale() of the same buffers as the fixture holds it (sha1 per plane and frame, frame 0 of the first rows in full),
the frames at which the reference's sums leave int32 included; one Tier-1 call per row; the line entry against the numpy restatement; the refusals and
the twin rule on the real library.  Nothing but that fixture is read: neither the reference's sources nor a library built from them."""
import pytest

import sws_gbrp as B

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", B.NAMES)
def test_gbrp_batched_on_the_device(mi355, name):
    p = B.check_batch(mi355.lib, name)
    assert p["gbrp"] == 1 and p["format"] == B.DST_GBRP and p["kernel"].startswith("planar_"), (name, p)


@pytest.mark.parametrize("name", B.NAMES)
def test_gbrp_tier1(mi355, name):
    # (the second picture reuses the context's device buffers)
    B.check_tier1(mi355.lib, name)


def test_gbrp_line_entry_on_the_device(mi355):
    assert B.check_line_entry(mi355.lib) == 4 * 4 * 2


def test_gbrp_refusals_and_twin_rule_on_the_device(mi355):
    lib = mi355.lib
    for what, e, with_coefs in B.refusal_cases():
        assert not B.create(lib, e, with_coefs), what
    assert not B.create_twin(lib, B.stored_entry("up_420_w130"), B.DST_GBRP)
    for n in B.NAMES:
        e = B.stored_entry(n)
        p, t = B.plan(lib, e), B.plan(lib, e, B.create_twin)
        assert p is not None and t is not None, n
        assert all(p[k] == t[k] for k in B.TWIN_KEYS), (n, p, t)
        assert (p["gbrp"], p["coefs"], p["format"], p["alpha"]) == (1, e.coefs, B.DST_GBRP, 0), (n, p)
        assert (t["gbrp"], t["coefs"], t["format"]) == (0, (0,) * 6, B.DST_YUV444P), n
