"""CPU: every compiled instance of the picture kernels of the device swscale path is launched by a row that a gpu-marked test compares with the
reference (tests/sws_instances.py).

The instance space is read from the emulated product library's symbol table (87 k_sws_generic, 168 k_sws_planar, 16 k_sws_ident1, 4 k_sws_ident1_yuy2,
6 k_sws_c24).  The census creates, on the emulator, every row the GPU tests of the thirteen feature tables launch, and every row of the table of
tests/sws_instances.py: the union of their keys is the whole space (minus UNREACHABLE, which is empty).  Every row of the new table names its key, and
the library's plan must give it; the rows stay small and are not all one narrow tile, asserted from the plan; every row equals the reference's own
sws_scale() of the same buffers through a guarded four-frame Tier-2 batch and, one per (source class, destination kind), through Tier 1; the committed
contexts are those of a live reference context."""
import os

import numpy as np
import pytest

import sws_instances as I
import sws_planar as P

HAVE_REF_LIB = os.path.exists(I.REF_LIB) or P.S.HAVE_REFERENCE
needs_ref = pytest.mark.skipif(not HAVE_REF_LIB, reason="oracle/_ref/libswsref.so is built by __graft_entry__.build() where the reference exists")
needs_sources = pytest.mark.skipif(not P.S.HAVE_REFERENCE, reason="needs the reference's sources (a fresh oracle/_ref/libswsref.so)")


@pytest.fixture(scope="module")
def ref_lib():
    """oracle/_ref/libswsref.so, made fresh where the reference's sources exist; None where there is no such library"""
    if P.S.HAVE_REFERENCE:
        I.make_fresh("_ref/libswsref.so")
    return I.REF_LIB if HAVE_REF_LIB else None


@pytest.fixture(scope="module")
def ref(ref_lib):
    return I.Ref(P.bind(ref_lib))


@pytest.fixture(scope="module")
def shapes_ref(ref_lib):
    """the live reference sws_shapes captures its contexts from, None without the library"""
    import sws_shapes as T
    return T.Ref(T.bind(ref_lib)) if ref_lib else None


@pytest.fixture(scope="module")
def space(emu):
    return I.instance_space()              # (the emu fixture has built the library)


@pytest.fixture(scope="module")
def plans(emu):
    return {name: I.plan(emu.lib, I.stored_entry(name)) for name in I.NAMES}


# ---- the instance space ------------------------------------------------------------------------------------------------------------
def test_instance_space_is_read_from_the_build(space):
    counts = {k: sum(1 for key in space if key[0] == k) for k in I.KERNELS}
    assert counts == I.COUNTS == {"generic": 87, "planar": 168, "ident1": 16, "ident1_yuy2": 4, "c24": 6}, counts
    assert {key[2] for key in space} == set(I.SRCS)
    # DEEP has no SEMI form, ALPHA is the RGB32 -> rgb32 pair alone: what sws_launch() says of itself
    assert not any(key[3] == "SEMI" and key[4] == "DEEP" for key in space)
    assert {key[:1] + key[2:] for key in space if key[6]} == {("generic", "RGB32", None, None, "rgb32", True)}


def test_symbol_keys_of_the_template_arguments_written_out():
    anon = "(anonymous namespace)::"
    assert I.symbol_key("generic", "48, 24, 4, %sSwsPx32A, false, true, 2" % anon) == ("generic", 2, "RGB32", None, None, "rgb32", True)
    assert I.symbol_key("generic", "40, 20, 5, %sSwsPxP010, true, false, 3" % anon) == ("generic", 1, "P010", None, None, "yuy2", False)
    assert I.symbol_key("generic", "28, 16, 8, unsigned char, false, true, 1") == ("generic", 0, "RGB24", None, None, "bgr24", False)
    assert I.symbol_key("planar", "40, 24, 64, unsigned char, true, true, false, true, false") == ("planar", 1, "NV", "SEMI", "RANGE", None, False)
    assert I.symbol_key("planar", "48, 48, 128, unsigned short, false, false, false, false, true") == ("planar", 2, "P16", "FULL", "DEEP", None, False)
    assert I.symbol_key("planar", "28, 16, 64, %sSwsPxYuy2, false, false, true, false, false" % anon) == ("planar", 0, "YUY2", "HALF", "PLAIN", None, False)
    assert I.symbol_key("ident1", "true, true, 1") == ("ident1", 1, "NV", None, None, "bgr24", False)
    assert I.symbol_key("ident1_yuy2", "3") == ("ident1_yuy2", 0, "YUY2", None, None, "yuy2", False)
    assert I.symbol_key("c24", "1, 2") == ("c24", 1, "P8", None, None, "rgb32", False)


def test_every_table_names_every_kernel(emu):
    """the plan queries of all the tables read ONE tuple of kernel names (sws_support.KERNELS): a packer's plan asked through an older table's
    plan_of() has its name (sws_nvsrc.plan_of raised IndexError for it)"""
    import sws_nv12 as N
    import sws_nvsrc as V
    import sws_sources as X
    import sws_yuy2dst as W
    import sws_yuy2src as Y
    assert len(P.S.KERNELS) == 13 and P.S.KERNELS[12] == "yuy2_pack" and X.KERNELS == P.S.KERNELS[:9]
    for name, module, kernel in (("s_422_yuyv", W, "yuy2_pack"), ("s_yuyv_420", Y, "yuy2_split")):
        for table in (X, N, V, Y, W):
            h = module.create(emu.lib, module.stored_entry(name))
            try:
                assert table.plan_of(emu.lib, h)["kernel"] == kernel, (name, table.__name__)
            finally:
                emu.lib.mi355_sws_destroy(I.C.c_void_p(h))


# ---- the census ------------------------------------------------------------------------------------------------------------------
def test_every_instance_is_launched_by_a_gpu_test(emu, space, plans, shapes_ref):
    """the keys of the rows the GPU tests of the feature tables launch (sws_instances.launched_rows: the GPU files' own lists), with those of this
    table's rows (test_instance_on_the_device runs every one), are the instance space.  Every such row is scaled and compared byte for byte with the
    reference (check_batch of its module)"""
    live = shapes_ref
    before = I.table_keys(emu.lib, live)
    own = {}
    for name, p in plans.items():
        own.setdefault(I.key_of(p), []).append(name)
    counts = "instances in the library: %d, reached before this table: %d, reached with it: %d" % (len(space), len(before), len(set(before) | set(own)))
    print(counts)
    assert set(before) <= space and set(own) <= space, (counts, [k for k in list(before) + list(own) if k not in space])
    # one row per unlaunched instance: none for an instance a feature table has, no two for one
    assert not set(own) & set(before), (counts, {I.key_text(k): (own[k], before[k]) for k in set(own) & set(before)})
    assert all(len(rows) == 1 for rows in own.values()), {I.key_text(k): rows for k, rows in own.items() if len(rows) > 1}
    assert len(I.UNREACHABLE) <= I.UNREACHABLE_CAP == 8 and set(I.UNREACHABLE) <= space
    assert not set(I.UNREACHABLE) & (set(before) | set(own)), "an instance listed as unreachable is reached"
    missing = space - set(before) - set(own) - set(I.UNREACHABLE)
    if live is None:
        # sws_shapes holds yuv420p -> rgb24 alone: whatever is left must be its
        assert all(k[2] == "P8" and k[5] == "rgb24" for k in missing), (counts, sorted(map(I.key_text, missing)))
        pytest.skip("sws_shapes captures its contexts from oracle/_ref/libswsref.so at run time: without the reference its contribution is left out (%s)" % counts)
    assert not missing, (counts, "no gpu-marked test launches", sorted(map(I.key_text, missing)))
    assert len(set(before) | set(own)) == len(space) - len(I.UNREACHABLE), counts


def test_nothing_is_listed_as_unreachable():
    """every instance has a row.  (An entry of UNREACHABLE needs a test of its reason here: the creator refuses every descriptor of that key the
    ladder of sws_instances.py's docstring can make, or the reference builds no such context.)"""
    assert I.UNREACHABLE == {}


def test_rows_name_their_instances(plans, space):
    for name in I.NAMES:
        p = plans[name]
        assert p is not None, (name, "refused")
        assert I.key_of(p) == I.key_for(name), (name, I.key_text(I.key_of(p)), "the row is there for", I.key_text(I.key_for(name)))
        assert I.plan_summary(p) == I.expected_plan(name), (name, I.plan_summary(p))
        assert I.key_for(name) in space, name
        lay, depth = I.SOURCES[I.cfg(name)[4]]
        fmt, bits = I.DSTS[I.cfg(name)[6]]
        assert (p["layout"], p["depth"], p["format"], p["dst_depth"], p["range"]) == (lay, depth, fmt, bits, I.expected_range(name)), (name, p)


def test_rows_are_small():
    for name in I.NAMES:
        sw, sh, dw, dh = I.cfg(name)[:4]
        assert sw <= 520 and sh <= 600 and dw <= 520 and dh <= 600, name
        assert sw % 2 == 0, name                         # no source reads behind its width: frame 3 of a batch is frame 0 whatever its padding holds


def test_rows_are_not_all_one_narrow_tile(plans):
    """from the plan, PER SOURCE CLASS (the reading of the rule that is meant here: one row of each kind among the class's rows, not one per instance —
    the table keeps the smallest picture that reaches an instance): a B or C row of a full tile and a partial one; a B or C row of an odd width; a
    horizontal reduction whose span is staged and one where it is not (either may be an instance-A row); a wide B or C row in the register-store
    form (narrow 0: a full tile and vertical banks of at most eight taps).  With 16 rows a tile B and C are reached at ratios of 5:4 to 5:2, where
    the bicubic banks already have at most eight taps: the rows that do so keep the bicubic flags of their neighbours, no bilinear row was needed"""
    for src in I.SRCS:
        rows = [(n, I.cfg(n), plans[n]) for n in I.NAMES if I.key_for(n)[2] == src and I.key_for(n)[0] in ("generic", "planar")]
        bc = [(n, c, p) for n, c, p in rows if I.key_for(n)[1] >= 1]
        assert any(c[2] >= 130 for n, c, p in bc), src
        assert any(c[2] % 2 for n, c, p in bc), src
        assert {p["hstaged"] for n, c, p in rows if c[0] > c[2]} == {0, 1}, src
        assert any(c[2] >= 130 and p["narrow"] == 0 for n, c, p in bc), src


def test_batch_layouts_reach_the_alignment_classes():
    least = {1: 1, 2: 2, 4: 4}
    for name in I.NAMES:
        g = I.granule(name)
        lay = I.src_layouts(name)
        assert all(I.align_class(o, st) == 16 for o, st in lay[0]), name
        assert all(I.align_class(o, st) == 4 for o, st in lay[1]), name
        assert all(I.align_class(o, st) == least[g] and o % 16 == least[g] for o, st in lay[2]), name
        assert all(a[1] != b[1] for a, b in zip(lay[0], lay[3])), name                       # frame 3: other strides
        assert all(o % g == 0 and st % g == 0 for f in lay for o, st in f), name
        # the destination rows of the four frames start on 16-byte multiples, on 4-byte ones, and at the writer's least aligned position (a 32-bit
        # row: a 4-byte multiple)
        e = I.stored_entry(name)
        rows = {I.align_class(o + y * st, 0) for f in I.dst_layout(e)[0] for (o, st), (_, h) in zip(f, e.out_sizes()) for y in range(h)}
        assert rows >= ({16, 4} if 33 <= e.fmt <= 36 else ({16, 4, 2} if e.dst_depth > 8 else {16, 4, 1})), (name, rows)


# ---- the committed contexts -------------------------------------------------------------------------------------------------------
def test_the_fixture_is_small_and_shares_its_banks():
    assert os.path.getsize(I.CONTEXTS) < 1_000_000
    with np.load(I.CONTEXTS) as z:
        pool = [k for k in z.files if k.startswith("pool/")]
        assert len(pool) < len(I.NAMES) * len(I.POOLED) // 3, len(pool)
        assert all(len(z[n + "/refs"]) == len(I.POOLED) for n in I.NAMES)


@needs_sources
def test_committed_contexts_match_the_reference(ref):
    """every row is opened by the reference and described as the table expects (Ref.entry asserts it); the committed arrays — banks, LUTs and dither
    rows included — are those"""
    for name in I.NAMES:
        assert I.stored_entry(name).same(ref.entry(name)), name


# ---- parity with the reference ------------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("kinds", I.ORDERS)
@pytest.mark.parametrize("name", I.NAMES)
def test_emulated_instance(emu, ref, plans, name, kinds):
    p = I.check_batch(emu.lib, ref, name, kinds=kinds)
    assert p == plans[name] and I.key_of(p) == I.key_for(name), name


@needs_ref
@pytest.mark.parametrize("name", I.TIER1)
def test_emulated_tier1(emu, ref, name):
    I.check_tier1(emu.lib, ref, name)


def test_tier1_rows_cover_every_source_class_and_destination_kind_and_every_small_kernel():
    tile = [n for n in I.NAMES if I.key_for(n)[0] in ("generic", "planar")]
    small = [n for n in I.NAMES if n not in tile]
    pairs = {(I.key_for(n)[2], I.dst_kind(I.key_for(n))) for n in tile}
    assert {(I.key_for(n)[2], I.dst_kind(I.key_for(n))) for n in I.TIER1 if n in tile} == pairs
    # the five rows of k_sws_ident1 / k_sws_c24 go through both checks, whatever tile row shares their source class and destination
    assert len(small) == 5 and set(small) <= set(I.TIER1)
    assert len(I.TIER1) == len(pairs) + len(small)


def test_both_picture_orders_put_every_picture_with_x_content_on_every_load_form():
    """noise or the ramp — the pictures that vary along x — lies in frame 0 (16-byte pieces), in frame 1 (dwords) and in frame 2 (the least aligned
    position) in one order or the other; the extreme picture, which tells nothing of x, never stands alone for a form"""
    assert all(set(o) == set(I.KINDS) for o in I.ORDERS)
    for frame in range(3):
        assert {o[frame] for o in I.ORDERS} & {"noise", "ramp"}, frame
    assert {o[2] for o in I.ORDERS} >= {"noise"}
    # the pictures do vary along x and between the samples of a pixel; the extreme one along y alone
    for name in ("pb_rgb24_semi_range_128x48_131x48", "pc_p010_semi_plain_64x120_64x48", "gb_yuy2_yuy2_64x84_64x48"):
        for (w, h, _, _, unit), noise, ramp, ext in zip(I.src_planes(name), *(I.picture(name, k, frame=2) for k in I.KINDS)):
            assert len(np.unique(ramp[0, :w])) > w // (2 * unit) and (ramp[:, :w] == ramp[0, :w]).all(), name
            assert unit == 1 or (ramp[0, 0:w:unit] != ramp[0, 1:w:unit]).all(), name
            assert len(np.unique(noise[:, :w])) > 32, name
            assert (ext[0::2, :w] == ext[0, 0]).all() and (ext[1::2, :w] == 0).all() and ext[0, 0] > 0, name


@needs_ref
def test_the_comparison_notices_one_wrong_byte(emu, ref, monkeypatch):
    """check_batch against a reference whose last frame has ONE byte off, in the last row of the last plane"""
    name = "pc_nv_semi_range_64x120_64x48"
    real = I.Ref.scale
    calls = []

    def off_by_one(self, name, planes, sizes, pad=8):
        out = real(self, name, planes, sizes, pad)
        calls.append(1)
        if len(calls) == 4:
            out[-1][-1, sizes[-1][0] - 1] ^= 1
        return out
    monkeypatch.setattr(I.Ref, "scale", off_by_one)
    with pytest.raises(AssertionError, match="rows"):
        I.check_batch(emu.lib, ref, name)
    assert len(calls) == 4
