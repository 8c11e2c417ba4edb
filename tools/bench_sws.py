#!/usr/bin/env python3
"""Throughput of the swscale kernels on SURVEY.md §8d config 5 (not the headline metric; numbers go
to DESIGN.md): batch of device-resident pictures, HIP events around K launches, algorithmic bytes =
source planes read once + RGB24 written once.  Also times the CPU oracle on one picture."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import providers  # noqa: E402
import sws_support as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--configs", default="hd_special,hd_generic,uhd_to_hd")
    ap.add_argument("--planar", action="store_true",
                    help="planar yuv420p 2160p -> 1080p (k_sws_planar) beside the rgb24 uhd_to_hd kernel, alternating, at 32 and 256 pictures per launch")
    ap.add_argument("--sources", action="store_true",
                    help="the deeper / wider sources (mi355_sws_create_src) beside the 8-bit yuv420p point of the same shape, alternating: 2160p -> 1080p "
                         "rgb24 from yuv420p10le, 1080p unscaled generic rgb24 from yuv420p10le and from yuv422p; --frames pictures per launch")
    ap.add_argument("--nv12", action="store_true",
                    help="NV12 destinations beside the yuv420p destination of the same shape (2160p -> 1080p from 8 bits, 1080p equal size from 10 "
                         "bits), the unscaled packer beside k_sws_c24, and with --other-lib the three existing points; 32 and 512 pictures per "
                         "launch, 3 warm-up + --steps launches a round, alternating, median of 3 rounds")
    ap.add_argument("--nvsrc", action="store_true",
                    help="NV12 sources (mi355_sws_create_src_layout) beside the yuv420p twin of the same shape on --other-lib (the parent commit's "
                         "build; this build without it): 2160p -> 1080p rgb24, 1080p -> rgb24 at equal size (ident1_x), 2160p -> 1080p nv12, the "
                         "unscaled splitter beside the packer at 1080p, one twin a second time in another allocation (A/A), and with --other-lib "
                         "the three existing points; 32 and 512 pictures per launch, 3 warm-up + --steps launches a round, alternating, median of 3 rounds")
    ap.add_argument("--rgbsrc", action="store_true",
                    help="packed rgb24 sources (mi355_sws_create_src_layout) beside the 8-bit yuv444p twin — the same three bytes a pixel in, the same "
                         "destination out — on --other-lib (the parent commit's build; this build without it): 2160p -> 1080p yuv420p, nv12 and rgb24, "
                         "1080p -> yuv420p at equal size, each twin a second time in another allocation (A/A), and with --other-lib the three "
                         "existing points; 32 and 512 pictures per launch, 3 warm-up + --steps launches a round, alternating, median of 3 rounds")
    ap.add_argument("--range", action="store_true",
                    help="range conversion (mi355_sws_create_src_layout_range) beside THE SAME descriptor created with range 0 on the same build — identical "
                         "banks and traffic: 1080p yuvj420p -> yuv420p and yuv420p -> yuvj420p at equal size, 2160p yuvj420p -> 1080p yuv420p and nv12, "
                         "1080p rgb24 -> yuvj420p; the partner a second time in another allocation (A/A), with --other-lib also on that build, and the "
                         "reference's single-thread sws_scale(); 32 and 512 pictures per launch, 3 warm-up + --steps launches a round, alternating, "
                         "median of 3 rounds")
    ap.add_argument("--deepdst", action="store_true",
                    help="10-bit planar destinations (mi355_sws_create_src_layout_range_depth) beside THE SAME descriptor created with depth 8 on the same "
                         "build — identical banks and source traffic, half the destination bytes: 2160p -> 1080p yuv420p10le and 1080p 4:2:0 -> "
                         "yuv422p10le at equal size, each from yuv420p10le, yuv420p and nv12; the twin a second time in another allocation (A/A); 32 "
                         "and 512 pictures per launch, 3 warm-up + --steps launches a round, alternating, median of 3 rounds")
    ap.add_argument("--packeddst", action="store_true",
                    help="bgr24 and 32-bit (bgra) destinations beside THE SAME descriptor created as rgb24 on the same build — identical banks, LUTs and "
                         "source traffic; bgr24 the same destination bytes, bgra a third more: 2160p -> 1080p from yuv420p, nv12 and yuv420p10le, 1080p at "
                         "equal size through k_sws_ident1 and through the special converter; the twin a second time in another allocation (A/A); 32 and "
                         "512 pictures per launch, 3 warm-up + --steps launches a round, alternating, median of 3 rounds")
    ap.add_argument("--rgb32src", action="store_true",
                    help="32-bit (bgra) sources beside THE SAME descriptor with an rgb24 source on the same build — identical banks and destination, a "
                         "third more source bytes: 2160p -> 1080p to yuv420p, nv12 and bgra, 1080p -> yuv420p and nv12 at equal size; 2160p -> 1080p bgra -> "
                         "bgra with alpha beside the same context with alpha 0 (equal bytes); the twin a second time in another allocation (A/A), with "
                         "--other-lib also on that build (the parent commit's) together with its 2160p -> 1080p yuv420p -> bgra point; 32 and 512 pictures "
                         "per launch, 3 warm-up + --steps launches a round, alternating, median of 3 rounds")
    ap.add_argument("--yuy2src", action="store_true",
                    help="the unscaled splitter of the packed 4:2:2 sources beside k_sws_nv12_split at the same size on the same build: 1080p uyvy422 -> "
                         "yuv420p (3.5 bytes a pixel against the twin's 3) and 1080p yuyv422 -> yuv422p (4 against 3); the twin a second time in another "
                         "allocation (A/A); 32 and 512 pictures per launch, 3 warm-up + --steps launches a round, alternating, median of --rounds rounds")
    ap.add_argument("--yuy2dst", action="store_true",
                    help="packed 4:2:2 destinations beside THE SAME descriptor with an rgb24 destination on the same build — identical banks and source, two "
                         "bytes a pixel written where rgb24 writes three, no table lookups: 2160p -> 1080p yuv420p -> yuyv422 and nv12 -> uyvy422, 1080p "
                         "yuv420p -> yuyv422 at equal size (k_sws_ident1); the unscaled packer 1080p yuv422p -> yuyv422 beside k_sws_nv12_pack at the same "
                         "size (4 bytes a pixel against 3); the twin a second time in another allocation (A/A); 32 and 512 pictures per launch, 3 warm-up + "
                         "--steps launches a round, alternating, median of --rounds rounds")
    ap.add_argument("--p010", action="store_true",
                    help="P010 sources beside THE SAME descriptor as a yuv420p10le source on the word >> 6 planes — identical banks, destination and source "
                         "bytes: 2160p -> 1080p p010le -> rgb24 and -> yuv420p10le, 1080p p010le -> nv12 at equal size; the twin a second time in another "
                         "allocation (A/A), with --other-lib also on that build (the parent commit's); and a plain device copy of the source bytes (the "
                         "twin plus that copy is the cheapest two-step route); 32 and 512 pictures per launch, 3 warm-up + --steps launches a round, "
                         "alternating, median of --rounds rounds")
    ap.add_argument("--fast-bilinear", action="store_true",
                    help="SWS_FAST_BILINEAR contexts (mi355_sws_create_fast_bilinear) beside (a) the SWS_BILINEAR context of the same geometry on the bank-driven "
                         "kernels and (b) the same arithmetic restated as two-tap banks for the existing creator: 2160p -> 1080p and 1080p -> 2160p yuv420p to "
                         "rgb24 and to yuv420p; (a) a second time in another allocation (A/A); 32 and 512 pictures per launch, 3 warm-up + --steps launches a "
                         "round, alternating, median of --rounds rounds")
    ap.add_argument("--gbrp", action="store_true",
                    help="gbrp destinations (mi355_sws_create_gbrp) from yuv420p beside (a) the yuv444p twin of the same descriptor — the same passes, LDS and bytes "
                         "written, no matrix — and (b) the rgb24 destination of the same geometry: 2160p -> 1080p, 1080p -> 2160p and 1080p -> 640x360; (a) a "
                         "second time in another allocation (A/A); 32 and 512 pictures per launch, 3 warm-up + --steps launches a round, alternating, median of "
                         "--rounds rounds")
    ap.add_argument("--other-lib", default=None,
                    help="--nv12 / --nvsrc / --rgbsrc / --range / --rgb32src / --p010: a second build of libmi355dsp.so (the parent commit's): the contexts it can build are timed on it too, alternating")
    ap.add_argument("--rounds", type=int, default=5, help="--planar / --sources / --yuy2src / --yuy2dst: alternating rounds (the median is reported)")
    a = ap.parse_args()
    prov = providers.mi355()
    lib = prov.lib
    lib.mi355_event_create.restype = C.c_void_p
    lib.mi355_event_elapsed_ms.restype = C.c_float
    if a.planar:
        return planar(a, lib)
    if a.sources:
        return sources(a, lib)
    if a.nv12:
        return nv12(a, lib)
    if a.nvsrc:
        return nvsrc(a, lib)
    if a.rgbsrc:
        return rgbsrc(a, lib)
    if a.range:
        return range_points(a, lib)
    if a.deepdst:
        return deepdst_points(a, lib)
    if a.packeddst:
        return packeddst_points(a, lib)
    if a.rgb32src:
        return rgb32src_points(a, lib)
    if a.yuy2src:
        return yuy2src_points(a, lib)
    if a.yuy2dst:
        return yuy2dst_points(a, lib)
    if a.p010:
        return p010_points(a, lib)
    if a.fast_bilinear:
        return fastbl_points(a, lib)
    if a.gbrp:
        return gbrp_points(a, lib)
    orc = S.oracle_backend(providers.oracle())
    for name in a.configs.split(","):
        ctx = S.load_context(name)
        d = ctx.desc
        pics = [S.picture(name, seed=s) for s in (1, 2)]
        batch = S.DeviceBatch(lib, ctx, pics, a.frames)
        for _ in range(3):
            batch.run()
        lib.mi355_sync(None)
        e0, e1 = lib.mi355_event_create(), lib.mi355_event_create()
        lib.mi355_event_record(C.c_void_p(e0), None)
        for _ in range(a.steps):
            batch.run()
        lib.mi355_event_record(C.c_void_p(e1), None)
        lib.mi355_sync(None)
        ms = lib.mi355_event_elapsed_ms(C.c_void_p(e0), C.c_void_p(e1)) / a.steps
        bytes_frame = d.srcW * d.srcH + 2 * d.chrSrcW * d.chrSrcH + d.dstW * d.dstH * 3
        fps = a.frames / (ms * 1e-3)
        t = time.time()
        orc.scale(ctx, pics[0])
        cpu = time.time() - t
        print(json.dumps({"workload": name, "frames_per_launch": a.frames, "ms_per_launch": ms, "frames_per_s": fps,
                          "algorithmic_bytes_per_frame": bytes_frame, "achieved_GBps": fps * bytes_frame / 1e9,
                          "frac_of_8TBps": fps * bytes_frame / 8e12, "cpu_oracle_frames_per_s_1core": 1.0 / cpu}))
        batch.close()


def time_ms(lib, run, steps):
    for _ in range(3):
        run()
    lib.mi355_sync(None)
    e0, e1 = lib.mi355_event_create(), lib.mi355_event_create()
    lib.mi355_event_record(C.c_void_p(e0), None)
    for _ in range(steps):
        run()
    lib.mi355_event_record(C.c_void_p(e1), None)
    lib.mi355_sync(None)
    return lib.mi355_event_elapsed_ms(C.c_void_p(e0), C.c_void_p(e1)) / steps


def planar(a, lib):
    """yuv420p 3840x2160 -> 1920x1080 yuv420p (algorithmic bytes: the source planes read once + the destination planes written once) and the
    rgb24 uhd_to_hd context (source read once + RGB24 written once), in the same process, alternating launches of K steps; median of --rounds"""
    import statistics
    import sws_planar as P
    ref = P.Ref(P.bind(P.REF_LIB))
    name = "big_uhd_to_hd"
    pctx = P.context(ref, name)
    rctx = S.load_context("uhd_to_hd")
    pics = [P.picture(name, seed=s) for s in (1, 2)]
    for frames in (32, 256):
        rgb = S.DeviceBatch(lib, rctx, [S.picture("uhd_to_hd", seed=s) for s in (1, 2)], frames)
        handle = P.create(lib, pctx, "420")
        assert handle
        pb = P.Batch(lib, pctx, "420", [pics[f % 2] for f in range(frames)], dst_pads=(0,), gaps=(64,))
        t = {"planar": [], "rgb24": []}
        for _ in range(a.rounds):
            t["rgb24"].append(time_ms(lib, rgb.run, a.steps))
            t["planar"].append(time_ms(lib, lambda: pb.launch(handle), a.steps))
        d = pctx.desc
        cw, ch = (d.dstW + 1) // 2, (d.dstH + 1) // 2
        pbytes = d.srcW * d.srcH + 2 * d.chrSrcW * d.chrSrcH + d.dstW * d.dstH + 2 * cw * ch
        r = rctx.desc
        rbytes = r.srcW * r.srcH + 2 * r.chrSrcW * r.chrSrcH + r.dstW * r.dstH * 3
        for kind, nbytes in (("planar", pbytes), ("rgb24", rbytes)):
            ms = statistics.median(t[kind])
            us = ms * 1e3 / frames
            print(json.dumps({"workload": "uhd_to_hd_" + ("yuv420p" if kind == "planar" else "rgb24"), "frames_per_launch": frames,
                              "ms_per_launch": ms, "us_per_picture": us, "algorithmic_bytes_per_frame": nbytes,
                              "achieved_GBps": nbytes / us * 1e-3, "frac_of_8TBps": nbytes / us * 1e-3 / 8000.0,
                              "ms_rounds": [round(x, 4) for x in t[kind]]}))
        pb.close()
        lib.mi355_sws_destroy(C.c_void_p(handle))
        rgb.close()


class SourceBatch:
    """`frames` pictures of one entry of tests/sws_sources.py resident in HBM, each with its own source planes (the first two uploaded, the
    rest device-side copies) and its own rgb24 destination"""

    def __init__(self, lib, X, e, pics, frames, create=None, bpp=3):
        self.lib, self.bufs, self.n = lib, [], frames
        lib.mi355_malloc.restype = C.c_void_p
        lib.mi355_malloc.argtypes = [C.c_size_t]
        lib.mi355_free.argtypes = [C.c_void_p]
        for f in ("mi355_memcpy_h2d", "mi355_memcpy_d2d"):
            getattr(lib, f).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        d = e.ctx.desc
        arr = (S.SwsFrame * frames)()
        self.src_bytes = 0
        for p in range(len(pics[0])):                 # (two planes for an NV12 / NV21 source)
            psz = pics[0][p].nbytes
            self.src_bytes += psz
            base = self.alloc(frames * psz + 64)
            for g, pic in enumerate(pics):
                lib.mi355_memcpy_h2d(base + g * psz, pic[p].ctypes.data, psz)
            done = len(pics)
            while done < frames:
                k = min(done, frames - done)
                lib.mi355_memcpy_d2d(base + done * psz, base, k * psz)
                done += k
            for f in range(frames):
                arr[f].src[p], arr[f].src_stride[p] = base + f * psz, pics[0][p].strides[0]
        self.dst_bytes = d.dstW * bpp * d.dstH                # (bpp 4: a 32-bit packed destination, tests/sws_packeddst.py)
        dst = self.alloc(frames * self.dst_bytes + 64)
        for f in range(frames):
            arr[f].dst, arr[f].dst_stride = dst + f * self.dst_bytes, d.dstW * bpp
        self.d_frames = self.alloc(C.sizeof(arr))
        lib.mi355_memcpy_h2d(self.d_frames, C.addressof(arr), C.sizeof(arr))
        self.handle = (create or X.create)(lib, e)
        assert self.handle
        lib.mi355_sws_scale_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]

    def alloc(self, n):
        p = self.lib.mi355_malloc(n)
        assert p
        self.bufs.append(p)
        return p

    def run(self):
        self.lib.mi355_sws_scale_frames_dev(C.c_void_p(self.handle), C.c_void_p(self.d_frames), self.n, None)

    def close(self):
        self.lib.mi355_sws_destroy(C.c_void_p(self.handle))
        for p in self.bufs:
            self.lib.mi355_free(p)


def sources(a, lib):
    """The new sources beside the 8-bit yuv420p context of the same shape, in one process, alternating launches of --steps; medians of --rounds.
    Algorithmic bytes: the source planes read once (2 bytes a sample above 8 bits) + RGB24 written once.  The contexts come from the
    reference's libswscale (oracle/_ref/libswsref.so), whose own sws_scale() of one picture is timed beside (one core)."""
    import statistics
    import numpy as np
    import sws_planar as P
    import sws_sources as X
    ref = X.Ref(P.bind(X.REF_LIB))
    points = [("uhd_to_hd", [("yuv420p10le", ("420", 10))], (3840, 2160, 1920, 1080)),
              ("hd_generic", [("yuv420p10le", ("420", 10)), ("yuv422p", ("422", 8))], (1920, 1080, 1920, 1080))]
    for base_name, news, (sw, sh, dw, dh) in points:
        rctx = S.load_context(base_name)
        batches = {"yuv420p": S.DeviceBatch(lib, rctx, [S.picture(base_name, seed=s) for s in (1, 2)], a.frames)}
        nbytes = {"yuv420p": sw * sh * 3 // 2 + dw * dh * 3}
        cpu = {}
        for label, (sub, depth) in news:
            shape = (sw, sh, dw, dh, sub, depth, "rgb", 1, 1, 1)
            c = ref.open_shape(*shape)
            e = ref.describe(c)
            assert e is not None, label
            X.SHAPES["_bench"] = shape
            pics = [X.picture("_bench", seed=s) for s in (1, 2)]
            pics = [[np.ascontiguousarray(pl) for pl in pic] for pic in pics]
            t0 = time.time()
            ref.scale_ctx(c, pics[0], e.out_sizes(), pad=0)
            cpu[label] = time.time() - t0
            ref.free(c)
            b = SourceBatch(lib, X, e, pics, a.frames)
            batches[label], nbytes[label] = b, b.src_bytes + b.dst_bytes
            b.plan = X.plan_of(lib, b.handle)
        t = {k: [] for k in batches}
        for _ in range(a.rounds):
            for k, b in batches.items():
                t[k].append(time_ms(lib, b.run, a.steps))
        for k, b in batches.items():
            ms = statistics.median(t[k])
            us = ms * 1e3 / a.frames
            out = {"workload": "%s_from_%s" % (base_name, k), "frames_per_launch": a.frames, "ms_per_launch": ms, "us_per_picture": us,
                   "frames_per_s": 1e6 / us, "algorithmic_bytes_per_frame": nbytes[k], "achieved_GBps": nbytes[k] / us * 1e-3,
                   "frac_of_8TBps": nbytes[k] / us * 1e-3 / 8000.0, "ms_rounds": [round(x, 4) for x in t[k]]}
            if k in cpu:
                out["reference_sws_scale_frames_per_s_1core"] = 1.0 / cpu[k]
                out["kernel"], out["hstaged"] = b.plan["kernel"], b.plan["hstaged"]
            print(json.dumps(out), flush=True)
            b.close()


class PlaneBatch:
    """`frames` pictures for one context of the planar entry points resident in HBM: each its own source planes (the given pictures uploaded,
    the rest device-side copies) and its own two or three tightly pitched destination planes of `sizes` (bytes per row, rows)"""

    def __init__(self, lib, handle, pics, sizes, frames):
        import sws_planar as P
        self.lib, self.bufs, self.n, self.handle = lib, [], frames, handle
        assert handle
        lib.mi355_malloc.restype = C.c_void_p
        lib.mi355_malloc.argtypes = [C.c_size_t]
        lib.mi355_free.argtypes = [C.c_void_p]
        for f in ("mi355_memcpy_h2d", "mi355_memcpy_d2d"):
            getattr(lib, f).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        arr = (P.PlanarFrame * frames)()
        self.src_bytes = 0
        for p in range(len(pics[0])):                 # (two planes for an NV12 / NV21 source)
            psz = pics[0][p].nbytes
            self.src_bytes += psz
            base = self.alloc(frames * psz + 64)
            for g, pic in enumerate(pics):
                lib.mi355_memcpy_h2d(base + g * psz, pic[p].ctypes.data, psz)
            done = len(pics)
            while done < frames:
                k = min(done, frames - done)
                lib.mi355_memcpy_d2d(base + done * psz, base, k * psz)
                done += k
            for f in range(frames):
                arr[f].src[p], arr[f].src_stride[p] = base + f * psz, pics[0][p].strides[0]
        self.dst_bytes = sum(w * h for w, h in sizes)
        dst = self.alloc(frames * self.dst_bytes + 64)
        for f in range(frames):
            o = dst + f * self.dst_bytes
            for p, (w, h) in enumerate(sizes):
                arr[f].dst[p], arr[f].dst_stride[p] = o, w
                o += w * h
        self.d_frames = self.alloc(C.sizeof(arr))
        lib.mi355_memcpy_h2d(self.d_frames, C.addressof(arr), C.sizeof(arr))
        lib.mi355_sws_scale_planar_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]

    def alloc(self, n):
        p = self.lib.mi355_malloc(n)
        assert p
        self.bufs.append(p)
        return p

    def run(self):
        self.lib.mi355_sws_scale_planar_frames_dev(C.c_void_p(self.handle), C.c_void_p(self.d_frames), self.n, None)

    def close(self):
        self.lib.mi355_sws_destroy(C.c_void_p(self.handle))
        for p in self.bufs:
            self.lib.mi355_free(p)


def nv12(a, lib):
    """NV12 destinations beside the three-plane yuv420p destination of the same shape, the packer beside k_sws_c24, every context from the
    committed tables (tests/golden).  One process, the batches of a point alternating: 3 warm-up + --steps launches a round, median of 3
    rounds, at 32 and 512 pictures per launch.  Algorithmic bytes: the source planes read once + the destination planes written once.
    --other-lib: the contexts a second build of the library takes (not the NV12 ones of a build without them) run on it in the same
    alternation, and so do the three points of the default mode."""
    import statistics
    import numpy as np
    import sws_nv12 as N
    import sws_planar as P
    import sws_sources as X
    libs = {"this": lib}
    if a.other_lib:
        other = C.CDLL(os.path.abspath(a.other_lib))
        other.mi355_init.restype = C.c_int
        assert other.mi355_init(C.c_int(0)) == 0
        other.mi355_event_create.restype = C.c_void_p
        other.mi355_event_elapsed_ms.restype = C.c_float
        libs["other"] = other
    rounds = 3

    def contiguous(pic):
        return [np.ascontiguousarray(pl) for pl in pic]

    def report(point, frames, batches, nbytes, t, extra):
        for k in batches:
            ms = statistics.median(t[k])
            us = ms * 1e3 / frames
            out = {"workload": point + ":" + k, "frames_per_launch": frames, "ms_per_launch": ms, "us_per_picture": us,
                   "algorithmic_bytes_per_frame": nbytes[k], "achieved_GBps": nbytes[k] / us * 1e-3, "frac_of_8TBps": nbytes[k] / us * 1e-3 / 8000.0,
                   "ms_rounds": [round(x, 4) for x in t[k]]}
            out.update(extra.get(k, {}))
            print(json.dumps(out), flush=True)

    def alternate(batches):
        t = {k: [] for k in batches}
        for _ in range(rounds):
            for k, (l, b) in batches.items():
                t[k].append(time_ms(l, b.run, a.steps))
        return t

    for frames in (32, 512):
        # 2160p -> 1080p bicubic from 8-bit yuv420p: nv12 beside yuv420p
        e = N.stored_entry("big_uhd420d8_to_hd_nv12")
        pctx = P.stored_context("big_uhd_to_hd")
        pics = [contiguous(P.picture("big_uhd_to_hd", seed=s)) for s in (1, 2)]
        batches, extra = {}, {}
        for tag, l in libs.items():
            batches["yuv420p@" + tag] = (l, PlaneBatch(l, P.create(l, pctx, "420"), pics, P.plane_sizes(pctx, "420"), frames))
        batches["nv12@this"] = (lib, PlaneBatch(lib, N.create(lib, e), pics, e.out_sizes(), frames))
        extra["nv12@this"] = {"kernel": N.plan_of(lib, batches["nv12@this"][1].handle)["kernel"]}
        nbytes = {k: b.src_bytes + b.dst_bytes for k, (l, b) in batches.items()}
        report("uhd_to_hd_from_yuv420p", frames, batches, nbytes, alternate(batches), extra)
        for l, b in batches.values():
            b.close()
        # 1080p equal size from 10 bits: yuv420p10le -> nv12 beside yuv422p10le -> yuv420p (yuv420p10le -> yuv420p is a plane copy)
        e = N.stored_entry("big_hd420d10_to_nv12")
        pe = X.stored_entry("big_hd422d10_to_420")
        batches, extra = {}, {}
        ppics = [contiguous(X.picture("big_hd422d10_to_420", seed=s)) for s in (1, 2)]
        for tag, l in libs.items():
            batches["yuv422p10le_to_yuv420p@" + tag] = (l, PlaneBatch(l, X.create(l, pe), ppics, pe.out_sizes(), frames))
        npics = [contiguous(N.picture("big_hd420d10_to_nv12", seed=s)) for s in (1, 2)]
        batches["yuv420p10le_to_nv12@this"] = (lib, PlaneBatch(lib, N.create(lib, e), npics, e.out_sizes(), frames))
        extra["yuv420p10le_to_nv12@this"] = {"kernel": N.plan_of(lib, batches["yuv420p10le_to_nv12@this"][1].handle)["kernel"]}
        nbytes = {k: b.src_bytes + b.dst_bytes for k, (l, b) in batches.items()}
        report("hd_same_from_10bit", frames, batches, nbytes, alternate(batches), extra)
        for l, b in batches.values():
            b.close()
        # the packer beside k_sws_c24 (the nearest copy-shaped kernel)
        e = N.stored_entry("big_hd420d8_pack")
        kpics = [contiguous(N.picture("big_hd420d8_pack", seed=s)) for s in (1, 2)]
        sctx = S.load_context("hd_special")
        batches = {"nv12_pack@this": (lib, PlaneBatch(lib, N.create(lib, e), kpics, e.out_sizes(), frames)),
                   "c24@this": (lib, S.DeviceBatch(lib, sctx, [S.picture("hd_special", seed=s) for s in (1, 2)], frames))}
        d = sctx.desc
        nbytes = {"nv12_pack@this": 2 * (1920 * 1080 * 3 // 2), "c24@this": d.srcW * d.srcH + 2 * d.chrSrcW * d.chrSrcH + d.dstW * d.dstH * 3}
        report("hd_unscaled", frames, batches, nbytes, alternate(batches), {})
        for l, b in batches.values():
            b.close()
    if "other" in libs:
        for name in a.configs.split(","):
            ctx = S.load_context(name)
            d = ctx.desc
            pics = [S.picture(name, seed=s) for s in (1, 2)]
            batches = {tag: (l, S.DeviceBatch(l, ctx, pics, a.frames)) for tag, l in (("other", libs["other"]), ("this", lib))}
            nb = d.srcW * d.srcH + 2 * d.chrSrcW * d.chrSrcH + d.dstW * d.dstH * 3
            report(name, a.frames, batches, {k: nb for k in batches}, alternate(batches), {})
            for l, b in batches.values():
                b.close()


def nvsrc(a, lib):
    """NV12 sources beside their yuv420p twins (the same sizes, destination and flags: the same banks).  The contexts come from the reference's
    libswscale at run time (oracle/_ref/libswsref.so: mi355_sws_describe_fmt / mi355_sws_describe_src) — no full-size context is committed.
    The twin runs on --other-lib (the parent commit's build) where one is given; `twin#2` is the twin's context a second time with its own
    buffers: identical code in two allocations, the session's A/A spread.  The splitter's twin is the packer.  One process, the batches of a
    point alternating: 3 warm-up + --steps launches a round, median of 3 rounds, at 32 and 512 pictures per launch.  Algorithmic bytes: the
    source planes read once + the destination planes written once."""
    import statistics
    import numpy as np
    import sws_nv12 as N
    import sws_nvsrc as V
    import sws_planar as P
    import sws_sources as X
    libs = {"this": lib}
    if a.other_lib:
        other = C.CDLL(os.path.abspath(a.other_lib))
        other.mi355_init.restype = C.c_int
        assert other.mi355_init(C.c_int(0)) == 0
        other.mi355_event_create.restype = C.c_void_p
        other.mi355_event_elapsed_ms.restype = C.c_float
        libs["other"] = other
    twin_tag, twin_lib = ("parent", libs["other"]) if a.other_lib else ("this", lib)
    ref = V.Ref(P.bind(V.REF_LIB))
    rounds = 3
    # (point, srcW, srcH, dstW, dstH, destination)
    points = [("uhd_to_hd_rgb24", 3840, 2160, 1920, 1080, "rgb"), ("hd_same_rgb24", 1920, 1080, 1920, 1080, "rgb"),
              ("uhd_to_hd_nv12", 3840, 2160, 1920, 1080, "nv12"), ("hd_split", 1920, 1080, 1920, 1080, "420")]

    def batch(l, e, pics, frames, create):
        if e.fmt == 0:
            return SourceBatch(l, X, e, pics, frames, create=create)
        return PlaneBatch(l, create(l, e), pics, e.out_sizes(), frames)

    for frames in (32, 512):
        for point, sw, sh, dw, dh, dst in points:
            flags = ref.lib.ref_sws_flags_word(1, 1, 1)
            c = ref.open_formats(sw, sh, b"nv12", dw, dh, V.AV_DST[dst], flags)
            e = ref.describe(c)
            ref.free(c)
            # the twin: yuv420p in; the splitter's is the packer (yuv420p -> nv12 at equal size)
            tdst = "nv12" if point == "hd_split" else dst
            c = ref.open_formats(sw, sh, b"yuv420p", dw, dh, V.AV_DST[tdst], flags)
            t = ref.describe_src(c)
            ref.free(c)
            assert e is not None and t is not None, point
            t = N.Entry.of(t)
            V.SHAPES["_bench"] = (sw, sh, dw, dh, "nv12", dst, 1, 1, 1)
            X.SHAPES["_bench"] = (sw, sh, dw, dh, "420", 8, "rgb", 1, 1, 1)
            npics = [[np.ascontiguousarray(pl) for pl in V.picture("_bench", seed=s)] for s in (1, 2)]
            tpics = [[np.ascontiguousarray(pl) for pl in X.picture("_bench", seed=s)] for s in (1, 2)]
            batches = {"nv12_source@this": (lib, batch(lib, e, npics, frames, V.create)),
                       "twin@" + twin_tag: (twin_lib, batch(twin_lib, t, tpics, frames, X.create)),
                       "twin#2@" + twin_tag: (twin_lib, batch(twin_lib, t, tpics, frames, X.create))}
            plan = V.plan_of(lib, batches["nv12_source@this"][1].handle)
            extra = {"nv12_source@this": {"kernel": plan["kernel"], "hstaged": plan["hstaged"]}}
            nbytes = {k: b.src_bytes + b.dst_bytes for k, (l, b) in batches.items()}
            times = {k: [] for k in batches}
            for _ in range(rounds):
                for k, (l, b) in batches.items():
                    times[k].append(time_ms(l, b.run, a.steps))
            for k in batches:
                ms = statistics.median(times[k])
                us = ms * 1e3 / frames
                out = {"workload": point + ":" + k, "frames_per_launch": frames, "ms_per_launch": ms, "us_per_picture": us,
                       "algorithmic_bytes_per_frame": nbytes[k], "achieved_GBps": nbytes[k] / us * 1e-3, "frac_of_8TBps": nbytes[k] / us * 1e-3 / 8000.0,
                       "ms_rounds": [round(x, 4) for x in times[k]]}
                out.update(extra.get(k, {}))
                print(json.dumps(out), flush=True)
            for l, b in batches.values():
                b.close()
    if "other" in libs:
        for name in a.configs.split(","):
            ctx = S.load_context(name)
            d = ctx.desc
            pics = [S.picture(name, seed=s) for s in (1, 2)]
            batches = {tag: (l, S.DeviceBatch(l, ctx, pics, a.frames)) for tag, l in (("parent", libs["other"]), ("this", lib))}
            nb = d.srcW * d.srcH + 2 * d.chrSrcW * d.chrSrcH + d.dstW * d.dstH * 3
            times = {k: [] for k in batches}
            for _ in range(rounds):
                for k, (l, b) in batches.items():
                    times[k].append(time_ms(l, b.run, a.steps))
            for k in batches:
                ms = statistics.median(times[k])
                print(json.dumps({"workload": name + ":" + k, "frames_per_launch": a.frames, "ms_per_launch": ms, "algorithmic_bytes_per_frame": nb,
                                  "ms_rounds": [round(x, 4) for x in times[k]]}), flush=True)
            for l, b in batches.values():
                b.close()


def rgbsrc(a, lib):
    """Packed rgb24 sources beside their traffic twins: the 8-bit yuv444p source of the same sizes, destination and flags reads the same three
    bytes a pixel and writes the same output.  The contexts come from the reference's libswscale at run time (oracle/_ref/libswsref.so:
    mi355_sws_describe_fmt / mi355_sws_describe_src) — no full-size context is committed.  The twin runs on --other-lib (the parent commit's
    build) where one is given; `twin#2` is the twin's context a second time with its own buffers: identical code in two allocations, the
    session's A/A spread.  One process, the batches of a point alternating: 3 warm-up + --steps launches a round, median of 3 rounds, at 32
    and 512 pictures per launch.  Algorithmic bytes: the source planes read once + the destination planes written once."""
    import statistics
    import numpy as np
    import sws_nv12 as N
    import sws_planar as P
    import sws_rgbsrc as R
    import sws_sources as X
    libs = {"this": lib}
    if a.other_lib:
        other = C.CDLL(os.path.abspath(a.other_lib))
        other.mi355_init.restype = C.c_int
        assert other.mi355_init(C.c_int(0)) == 0
        other.mi355_event_create.restype = C.c_void_p
        other.mi355_event_elapsed_ms.restype = C.c_float
        libs["other"] = other
    twin_tag, twin_lib = ("parent", libs["other"]) if a.other_lib else ("this", lib)
    ref = R.Ref(P.bind(R.REF_LIB))
    rounds = 3
    # (point, srcW, srcH, dstW, dstH, destination)
    points = [("uhd_to_hd_yuv420p", 3840, 2160, 1920, 1080, "420"), ("uhd_to_hd_nv12", 3840, 2160, 1920, 1080, "nv12"),
              ("hd_same_yuv420p", 1920, 1080, 1920, 1080, "420"), ("uhd_to_hd_rgb24", 3840, 2160, 1920, 1080, "rgb")]

    def batch(l, e, pics, frames, create):
        if e.fmt == 0:
            return SourceBatch(l, X, e, pics, frames, create=create)
        return PlaneBatch(l, create(l, e), pics, e.out_sizes(), frames)

    for frames in (32, 512):
        for point, sw, sh, dw, dh, dst in points:
            flags = ref.lib.ref_sws_flags_word(1, 1, 1)
            c = ref.open_formats(sw, sh, b"rgb24", dw, dh, R.AV_DST[dst], flags)
            e = ref.describe(c)
            ref.free(c)
            c = ref.open_formats(sw, sh, b"yuv444p", dw, dh, R.AV_DST[dst], flags)
            t = ref.describe_src(c)
            ref.free(c)
            assert e is not None and t is not None, point
            t = N.Entry.of(t)
            R.SHAPES["_bench"] = (sw, sh, dw, dh, "rgb24", dst, 1, 1, 1, 0)
            X.SHAPES["_bench"] = (sw, sh, dw, dh, "444", 8, "rgb", 1, 1, 1)
            # (the packed pictures keep their spare line: the kernels never read it at an even width)
            rpics = [R.picture("_bench", seed=s) for s in (1, 2)]
            tpics = [[np.ascontiguousarray(pl) for pl in X.picture("_bench", seed=s)] for s in (1, 2)]
            batches = {"rgb24_source@this": (lib, batch(lib, e, rpics, frames, R.create)),
                       "twin@" + twin_tag: (twin_lib, batch(twin_lib, t, tpics, frames, X.create)),
                       "twin#2@" + twin_tag: (twin_lib, batch(twin_lib, t, tpics, frames, X.create))}
            plan = R.plan_of(lib, batches["rgb24_source@this"][1].handle)
            extra = {"rgb24_source@this": {"kernel": plan["kernel"], "hstaged": plan["hstaged"], "hsub": plan["hsub"]}}
            nbytes = {k: b.src_bytes + b.dst_bytes for k, (l, b) in batches.items()}
            times = {k: [] for k in batches}
            for _ in range(rounds):
                for k, (l, b) in batches.items():
                    times[k].append(time_ms(l, b.run, a.steps))
            for k in batches:
                ms = statistics.median(times[k])
                us = ms * 1e3 / frames
                out = {"workload": point + ":" + k, "frames_per_launch": frames, "ms_per_launch": ms, "us_per_picture": us,
                       "algorithmic_bytes_per_frame": nbytes[k], "achieved_GBps": nbytes[k] / us * 1e-3, "frac_of_8TBps": nbytes[k] / us * 1e-3 / 8000.0,
                       "ms_rounds": [round(x, 4) for x in times[k]]}
                out.update(extra.get(k, {}))
                print(json.dumps(out), flush=True)
            for l, b in batches.values():
                b.close()
    if "other" in libs:
        for name in a.configs.split(","):
            ctx = S.load_context(name)
            d = ctx.desc
            pics = [S.picture(name, seed=s) for s in (1, 2)]
            batches = {tag: (l, S.DeviceBatch(l, ctx, pics, a.frames)) for tag, l in (("parent", libs["other"]), ("this", lib))}
            nb = d.srcW * d.srcH + 2 * d.chrSrcW * d.chrSrcH + d.dstW * d.dstH * 3
            times = {k: [] for k in batches}
            for _ in range(rounds):
                for k, (l, b) in batches.items():
                    times[k].append(time_ms(l, b.run, a.steps))
            for k in batches:
                ms = statistics.median(times[k])
                print(json.dumps({"workload": name + ":" + k, "frames_per_launch": a.frames, "ms_per_launch": ms, "algorithmic_bytes_per_frame": nb,
                                  "ms_rounds": [round(x, 4) for x in times[k]]}), flush=True)
            for l, b in batches.values():
                b.close()


def range_points(a, lib):
    """Range conversion beside its partner: the same descriptor created with range 0 on the same build has identical banks and traffic and lacks
    only the step between the two passes.  The contexts come from the reference's libswscale at run time (oracle/_ref/libswsref.so:
    mi355_sws_describe_range) — no full-size context is committed.  `range0#2` is the partner a second time with its own buffers: the session's
    A/A spread; with --other-lib the partner also runs on that build (the parent commit's, through mi355_sws_create_src_layout).  Beside each
    point the reference's own single-thread sws_scale() of one picture.  One process, the batches of a point alternating: 3 warm-up + --steps
    launches a round, median of 3 rounds, at 32 and 512 pictures per launch.  Algorithmic bytes: sources read once + destinations written once."""
    import statistics
    import sws_nvsrc as V
    import sws_planar as P
    import sws_range as G
    other = None
    if a.other_lib:
        other = C.CDLL(os.path.abspath(a.other_lib))
        other.mi355_init.restype = C.c_int
        assert other.mi355_init(C.c_int(0)) == 0
        other.mi355_event_create.restype = C.c_void_p
        other.mi355_event_elapsed_ms.restype = C.c_float
    ref = G.Ref(P.bind(G.REF_LIB))
    rounds = 3
    # (point, srcW, srcH, dstW, dstH, source, its range, destination, its range)
    points = [("hd_same_yuvj420p_to_yuv420p", 1920, 1080, 1920, 1080, "yuv420p", 1, "yuv420p", 0),
              ("hd_same_yuv420p_to_yuvj420p", 1920, 1080, 1920, 1080, "yuv420p", 0, "yuv420p", 1),
              ("uhd_to_hd_yuvj420p_to_yuv420p", 3840, 2160, 1920, 1080, "yuv420p", 1, "yuv420p", 0),
              ("uhd_to_hd_yuvj420p_to_nv12", 3840, 2160, 1920, 1080, "yuv420p", 1, "nv12", 0),
              ("hd_same_rgb24_to_yuvj420p", 1920, 1080, 1920, 1080, "rgb24", 0, "yuv420p", 1)]
    cpu = {}
    for frames in (32, 512):
        for point, sw, sh, dw, dh, src, sr, dst, dr in points:
            row = (sw, sh, dw, dh, src, sr, dst, dr, 1, 1, 1)          # a row of tests/sws_range.py's table, not entered into it
            c = ref.open(row)
            e = ref.describe_range(c)
            assert e is not None and e.range == G.direction(row), point
            pics = [G.picture(row, "noise", seed=s) for s in (1, 2)]
            if point not in cpu:
                ref.scale_ctx(c, pics[0], e.out_sizes(), pad=0)
                t = time.time()
                for pic in pics:
                    ref.scale_ctx(c, pic, e.out_sizes(), pad=0)
                cpu[point] = len(pics) / (time.time() - t)
            ref.free(c)
            partner = e.edited(range=0)
            batches = {"ranged@this": (lib, PlaneBatch(lib, G.create(lib, e), pics, e.out_sizes(), frames)),
                       "range0@this": (lib, PlaneBatch(lib, G.create(lib, partner), pics, e.out_sizes(), frames)),
                       "range0#2@this": (lib, PlaneBatch(lib, G.create(lib, partner), pics, e.out_sizes(), frames))}
            if other:
                batches["range0@parent"] = (other, PlaneBatch(other, V.create(other, partner), pics, e.out_sizes(), frames))
            plan = G.plan_of(lib, batches["ranged@this"][1].handle)
            times = {k: [] for k in batches}
            for _ in range(rounds):
                for k, (l, b) in batches.items():
                    times[k].append(time_ms(l, b.run, a.steps))
            base = statistics.median(times["range0@this"])
            for k, (l, b) in batches.items():
                ms = statistics.median(times[k])
                us = ms * 1e3 / frames
                nb = b.src_bytes + b.dst_bytes
                print(json.dumps({"workload": point + ":" + k, "frames_per_launch": frames, "ms_per_launch": ms, "us_per_picture": us, "frames_per_s": 1e6 / us,
                                  "algorithmic_bytes_per_frame": nb, "achieved_GBps": nb / us * 1e-3, "frac_of_8TBps": nb / us * 1e-3 / 8000.0,
                                  "vs_range0": ms / base - 1.0, "kernel": plan["kernel"], "hstaged": plan["hstaged"], "range": plan["range"] if k == "ranged@this" else 0,
                                  "reference_sws_scale_frames_per_s_1core": cpu[point], "ms_rounds": [round(x, 4) for x in times[k]]}), flush=True)
            for l, b in batches.values():
                b.close()


def deepdst_points(a, lib, points=None, frame_counts=(32, 512)):
    """A 10-bit planar destination beside its twin: the same descriptor created with depth 8 on the same build has identical banks and source
    traffic and writes half the destination bytes.  The contexts come from the reference's libswscale at run time (oracle/_ref/libswsref.so:
    mi355_sws_describe_depth) — no full-size context is committed.  `depth8#2` is the twin a second time with its own buffers: the session's
    A/A spread.  One process, the batches of a point alternating: 3 warm-up + --steps launches a round, median of 3 rounds, at 32 and 512
    pictures per launch.  Algorithmic bytes: sources read once + destinations written once.  `bound`: the extra destination bytes over the
    twin's algorithmic bytes — what the deep context may cost if it moves them at the twin's achieved bandwidth (the A/A spread comes on top)."""
    import statistics
    import sws_deepdst as D
    import sws_planar as P
    ref = D.Ref(P.bind(D.REF_LIB))
    rounds = 3
    # (point, srcW, srcH, dstW, dstH, source, destination)
    points = points or [("uhd_to_hd_%s_to_yuv420p10le" % s, 3840, 2160, 1920, 1080, s, "yuv420p10le") for s in ("yuv420p10le", "yuv420p", "nv12")] + \
                       [("hd_same_%s_to_yuv422p10le" % s, 1920, 1080, 1920, 1080, s, "yuv422p10le") for s in ("yuv420p10le", "yuv420p", "nv12")]
    for frames in frame_counts:
        for point, sw, sh, dw, dh, src, dst in points:
            row = (sw, sh, dw, dh, src, dst, 1, 1, 1)                  # a row of tests/sws_deepdst.py's table, not entered into it
            c = ref.open(row)
            e = ref.describe_depth(c)
            ref.free(c)
            assert e is not None and e.dst_depth == D.dst_kind(row)[1], point
            pics = [D.picture(row, "noise", seed=s) for s in (1, 2)]
            twin = e.edited(dst_depth=8)
            batches = {"deep": PlaneBatch(lib, D.create(lib, e), pics, e.out_sizes(), frames),
                       "depth8": PlaneBatch(lib, D.create(lib, twin), pics, twin.out_sizes(), frames),
                       "depth8#2": PlaneBatch(lib, D.create(lib, twin), pics, twin.out_sizes(), frames)}
            plan = D.plan_of(lib, batches["deep"].handle)
            times = {k: [] for k in batches}
            for _ in range(rounds):
                for k, b in batches.items():
                    times[k].append(time_ms(lib, b.run, a.steps))
            base = statistics.median(times["depth8"])
            twin_bytes = batches["depth8"].src_bytes + batches["depth8"].dst_bytes
            for k, b in batches.items():
                ms = statistics.median(times[k])
                us = ms * 1e3 / frames
                nb = b.src_bytes + b.dst_bytes
                print(json.dumps({"workload": point + ":" + k, "frames_per_launch": frames, "ms_per_launch": ms, "us_per_picture": us, "frames_per_s": 1e6 / us,
                                  "algorithmic_bytes_per_frame": nb, "achieved_GBps": nb / us * 1e-3, "frac_of_8TBps": nb / us * 1e-3 / 8000.0,
                                  "vs_depth8": ms / base - 1.0, "bound": nb / twin_bytes - 1.0, "kernel": plan["kernel"], "hstaged": plan["hstaged"],
                                  "dst_depth": plan["dst_depth"] if k == "deep" else 8, "ms_rounds": [round(x, 4) for x in times[k]]}), flush=True)
            for b in batches.values():
                b.close()


def packeddst_points(a, lib, points=None, frame_counts=(32, 512)):
    """A bgr24 and a 32-bit (bgra) destination beside their twin: the same descriptor created as rgb24 on the same build has identical banks, LUTs
    and source traffic; bgr24 writes the same destination bytes, bgra a third more.  The contexts come from the reference's libswscale at run time
    (oracle/_ref/libswsref.so: mi355_sws_describe_packed) — no full-size context is committed.  `rgb24#2` is the twin a second time with its own
    buffers: the session's A/A spread.  One process, the batches of a point alternating: 3 warm-up + --steps launches a round, median of 3 rounds,
    at 32 and 512 pictures per launch.  Algorithmic bytes: sources read once + destinations written once.  `bound`: the extra destination bytes
    over the twin's algorithmic bytes — what the context may cost if it moves them at the twin's achieved bandwidth (0 for bgr24; the A/A spread
    comes on top)."""
    import statistics
    import sws_nvsrc as V
    import sws_packeddst as K
    import sws_planar as P
    import sws_sources as X
    ref = K.Ref(P.bind(K.REF_LIB))
    rounds = 3
    # (point, srcW, srcH, dstW, dstH, source, accurate_rnd / bitexact: 0 at equal size is the unscaled special converter)
    points = points or [("uhd_to_hd_%s" % s, 3840, 2160, 1920, 1080, s, 1) for s in ("yuv420p", "nv12", "yuv420p10le")] + \
                       [("hd_same_yuv420p_ident1", 1920, 1080, 1920, 1080, "yuv420p", 1), ("hd_same_yuv420p_special", 1920, 1080, 1920, 1080, "yuv420p", 0)]
    for frames in frame_counts:
        for point, sw, sh, dw, dh, src, acc in points:
            entries = {}
            for dst in ("bgr24", "bgra"):
                row = (sw, sh, dw, dh, src, dst, 1, acc, acc)          # a row of tests/sws_packeddst.py's table, not entered into it
                c = ref.open(row)
                entries[dst] = ref.describe_packed(c)
                ref.free(c)
                assert entries[dst] is not None and entries[dst].fmt == K.DSTS[dst], point
            pics = [K.picture(row, "noise", seed=s) for s in (1, 2)]
            e = entries["bgr24"]
            twin = V.Entry(e.ctx, e.depth, e.hsub, e.vsub, e.dither, 0, e.layout)     # bgr24 has the rgb24 tables (tests/test_sws_packeddst_emu.py)
            batches = {"bgr24": SourceBatch(lib, X, entries["bgr24"], pics, frames, create=K.create),
                       "bgra": SourceBatch(lib, X, entries["bgra"], pics, frames, create=K.create, bpp=4),
                       "rgb24": SourceBatch(lib, X, twin, pics, frames, create=K.create),
                       "rgb24#2": SourceBatch(lib, X, twin, pics, frames, create=K.create)}
            plan = K.plan_of(lib, batches["bgra"].handle)
            times = {k: [] for k in batches}
            for _ in range(rounds):
                for k, b in batches.items():
                    times[k].append(time_ms(lib, b.run, a.steps))
            base = statistics.median(times["rgb24"])
            twin_bytes = batches["rgb24"].src_bytes + batches["rgb24"].dst_bytes
            for k, b in batches.items():
                ms = statistics.median(times[k])
                us = ms * 1e3 / frames
                nb = b.src_bytes + b.dst_bytes
                print(json.dumps({"workload": point + ":" + k, "frames_per_launch": frames, "ms_per_launch": ms, "us_per_picture": us, "frames_per_s": 1e6 / us,
                                  "algorithmic_bytes_per_frame": nb, "achieved_GBps": nb / us * 1e-3, "frac_of_8TBps": nb / us * 1e-3 / 8000.0,
                                  "vs_rgb24": ms / base - 1.0, "bound": nb / twin_bytes - 1.0, "kernel": plan["kernel"], "hstaged": plan["hstaged"],
                                  "ms_rounds": [round(x, 4) for x in times[k]]}), flush=True)
            for b in batches.values():
                b.close()


def rgb32src_points(a, lib, points=None, frame_counts=(32, 512)):
    """A 32-bit (bgra) source beside its twin: the context of the same sizes, destination and flags from rgb24 on the same build has the same
    banks and destination traffic and reads three bytes a pixel where this one reads four; and the alpha form (bgra -> bgra with the source's alpha
    carried) beside the same context with alpha 0, which moves the same bytes.  The contexts come from the reference's libswscale at run time
    (oracle/_ref/libswsref.so: mi355_sws_describe_rgb32 / _fmt / _packed) — no full-size context is committed.  `twin#2` is the twin a second time
    with its own buffers: the session's A/A spread.  With --other-lib the twin also runs on that build (the parent commit's), and so does the
    2160p -> 1080p yuv420p -> bgra point of --packeddst on both builds: what existed before must not have moved.  One process, the batches of a
    point alternating: 3 warm-up + --steps launches a round, median of 3 rounds, at 32 and 512 pictures per launch.  Algorithmic bytes: sources
    read once + destinations written once.  `bound`: this context's algorithmic bytes over the twin's — what it may cost if it moves them at the
    twin's achieved bandwidth.  The last line sums the session up: `aa_session` — the largest A/A spread of its points — and under `miss` every
    row whose time exceeds its twin's times the byte ratio plus that spread."""
    import statistics
    import sws_packeddst as K
    import sws_planar as P
    import sws_rgb32src as Q
    import sws_rgbsrc as R
    other = None
    if a.other_lib:
        other = C.CDLL(os.path.abspath(a.other_lib))
        other.mi355_init.restype = C.c_int
        assert other.mi355_init(C.c_int(0)) == 0
        other.mi355_event_create.restype = C.c_void_p
        other.mi355_event_elapsed_ms.restype = C.c_float
    ref = Q.Ref(P.bind(Q.REF_LIB))
    rounds = 3
    # (point, srcW, srcH, dstW, dstH, destination of tests/sws_rgb32src.py)
    points = points or [("uhd_to_hd_yuv420p", 3840, 2160, 1920, 1080, "420"), ("uhd_to_hd_nv12", 3840, 2160, 1920, 1080, "nv12"),
                        ("uhd_to_hd_bgra", 3840, 2160, 1920, 1080, "bgra"), ("hd_same_yuv420p", 1920, 1080, 1920, 1080, "420"),
                        ("hd_same_nv12", 1920, 1080, 1920, 1080, "nv12")]

    def batch(l, e, pics, frames, create, **kw):
        if e.fmt == 0 or e.fmt >= 32:
            return SourceBatch(l, None, e, pics, frames, create=create, bpp=4 if e.fmt >= 33 else 3, **kw)
        return PlaneBatch(l, create(l, e), pics, e.out_sizes(), frames)

    rows = []

    def report(point, frames, batches, times, base_key, spread_keys, extra):
        base = statistics.median(times[base_key])
        spread = abs(statistics.median(times[spread_keys[1]]) / statistics.median(times[spread_keys[0]]) - 1.0)
        twin_bytes = batches[base_key][1].src_bytes + batches[base_key][1].dst_bytes
        for k, (l, b) in batches.items():
            ms = statistics.median(times[k])
            us = ms * 1e3 / frames
            nb = b.src_bytes + b.dst_bytes
            out = {"workload": point + ":" + k, "frames_per_launch": frames, "ms_per_launch": ms, "us_per_picture": us, "frames_per_s": 1e6 / us,
                   "algorithmic_bytes_per_frame": nb, "achieved_GBps": nb / us * 1e-3, "frac_of_8TBps": nb / us * 1e-3 / 8000.0,
                   "vs_twin": ms / base - 1.0, "bound": nb / twin_bytes - 1.0, "aa_spread": spread, "ms_rounds": [round(x, 4) for x in times[k]]}
            out.update(extra.get(k, {}))
            rows.append(out)
            print(json.dumps(out), flush=True)

    for frames in frame_counts:
        for point, sw, sh, dw, dh, dst in points:
            row = (sw, sh, dw, dh, "bgra", dst, 1, 1, 1, 0)            # a row of tests/sws_rgb32src.py's table, not entered into it
            c = ref.open(row)
            e = ref.describe_rgb32(c)
            ref.free(c)
            c = ref.open_twin(row)
            t = ref.describe_packed(c) if dst in Q.LAYOUTS else ref.describe_fmt(c)
            ref.free(c)
            assert e is not None and t is not None, point
            t = Q.Entry(t.ctx, t.depth, t.hsub, t.vsub, t.dither, t.fmt, t.layout)
            R.SHAPES["_bench"] = (sw, sh, dw, dh, "rgb24", "rgb", 1, 1, 1, 0)
            qpics = [Q.picture(row, "noise", seed=s) for s in (1, 2)]
            tpics = [R.picture("_bench", seed=s) for s in (1, 2)]
            batches = {"bgra_source": (lib, batch(lib, e, qpics, frames, lambda l, x: Q.create(l, x, alpha=0))),
                       "twin": (lib, batch(lib, t, tpics, frames, Q.create)), "twin#2": (lib, batch(lib, t, tpics, frames, Q.create))}
            if other:
                batches["twin@parent"] = (other, batch(other, t, tpics, frames, Q.create))
            plan = Q.plan_of(lib, batches["bgra_source"][1].handle)
            times = {k: [] for k in batches}
            for _ in range(rounds):
                for k, (l, b) in batches.items():
                    times[k].append(time_ms(l, b.run, a.steps))
            report(point, frames, batches, times, "twin", ("twin", "twin#2"), {"bgra_source": {"kernel": plan["kernel"], "hstaged": plan["hstaged"], "hsub": plan["hsub"]}})
            for l, b in batches.values():
                b.close()
        # the alpha form beside the same context with alpha 0: equal bytes
        row = (3840, 2160, 1920, 1080, "bgra", "bgra", 1, 1, 1, 0)
        c = ref.open(row)
        e = ref.describe_rgb32(c)
        ref.free(c)
        assert e is not None and e.alpha == 1
        qpics = [Q.picture(row, "noise", seed=s) for s in (1, 2)]
        mk = lambda al: (lib, batch(lib, e, qpics, frames, lambda l, x: Q.create(l, x, alpha=al)))    # noqa: E731
        batches = {"alpha": mk(1), "alpha0": mk(0), "alpha0#2": mk(0)}
        times = {k: [] for k in batches}
        for _ in range(rounds):
            for k, (l, b) in batches.items():
                times[k].append(time_ms(l, b.run, a.steps))
        report("uhd_to_hd_bgra_to_bgra", frames, batches, times, "alpha0", ("alpha0", "alpha0#2"), {})
        for l, b in batches.values():
            b.close()
        if other:
            # what --packeddst has as its headline, on both builds
            krow = (3840, 2160, 1920, 1080, "yuv420p", "bgra", 1, 1, 1)
            kref = K.Ref(P.bind(K.REF_LIB))
            c = kref.open(krow)
            ke = kref.describe_packed(c)
            kref.free(c)
            kpics = [K.picture(krow, "noise", seed=s) for s in (1, 2)]
            batches = {"this": (lib, SourceBatch(lib, None, ke, kpics, frames, create=K.create, bpp=4)),
                       "this#2": (lib, SourceBatch(lib, None, ke, kpics, frames, create=K.create, bpp=4)),
                       "parent": (other, SourceBatch(other, None, ke, kpics, frames, create=K.create, bpp=4))}
            times = {k: [] for k in batches}
            for _ in range(rounds):
                for k, (l, b) in batches.items():
                    times[k].append(time_ms(l, b.run, a.steps))
            report("packeddst_uhd_to_hd_yuv420p_to_bgra", frames, batches, times, "parent", ("this", "this#2"), {})
            for l, b in batches.values():
                b.close()
    aa = max(r["aa_spread"] for r in rows)
    miss = ["%s@%d %+.1f%% (bound %+.1f%%)" % (r["workload"], r["frames_per_launch"], 100 * r["vs_twin"], 100 * (r["bound"] + aa)) for r in rows if r["vs_twin"] > r["bound"] + aa]
    print(json.dumps({"summary": "rgb32src", "aa_session": aa, "points": len(rows), "miss": miss}), flush=True)


def yuy2src_points(a, lib, points=None, frame_counts=(32, 512), scaled=None):
    """The unscaled splitter of the packed 4:2:2 sources (k_sws_yuy2_split) beside k_sws_nv12_split at the same size — the one kernel of the same
    kind: a de-interleaving copy without banks or LDS.  It moves 3 bytes a pixel (nv12 -> yuv420p: 1.5 in, 1.5 out); uyvy422 -> yuv420p moves 3.5
    (2 in, 1.5 out) and yuyv422 -> yuv422p 4 (2 in, 2 out): `bound` is that byte ratio — what the point may cost at the twin's achieved bandwidth.
    The contexts come from the reference's libswscale at run time (oracle/_ref/libswsref.so: mi355_sws_describe_yuy2 / _fmt) — no full-size
    context is committed.  `twin#2` is the twin a second time with its own buffers: the session's A/A spread.  One process, the batches of a point
    alternating: 3 warm-up + --steps launches a round, median of --rounds rounds, at 32 and 512 pictures per launch.  Algorithmic bytes: the source
    read once + the destination planes written once.  The last line sums the session up: `aa_session` — the largest A/A spread of its points — and
    under `miss` every row whose time exceeds its twin's times the byte ratio plus that spread.
    The scaler's points (2160p -> 1080p yuyv422 -> yuv420p, uyvy422 -> nv12, uyvy422 -> bgra, and 1080p yuyv422 -> bgra at equal size: k_sws_ident1_yuy2)
    run beside their yuv422p twin — the context of the SAME descriptor as an 8-bit planar 4:2:2 source on the de-interleaved planes: equal bytes a pixel
    (2 in both), so the bound is the twin's time."""
    import statistics
    import numpy as np
    import sws_nvsrc as V
    import sws_planar as P
    import sws_yuy2src as Y
    ref = Y.Ref(P.bind(Y.REF_LIB))
    vref = V.Ref(ref.lib)
    # (point, srcW, srcH, source, destination of tests/sws_yuy2src.py)
    points = points or [("hd_split_uyvy_yuv420p", 1920, 1080, "uyvy", "420"), ("hd_split_yuyv_yuv422p", 1920, 1080, "yuyv", "422")]
    # (point, srcW, srcH, dstW, dstH, source, destination): the scaler's points and the ident1 point
    scaled = scaled if scaled is not None else [("uhd_to_hd_yuyv_yuv420p", 3840, 2160, 1920, 1080, "yuyv", "420"), ("uhd_to_hd_uyvy_nv12", 3840, 2160, 1920, 1080, "uyvy", "nv12"),
              ("uhd_to_hd_uyvy_bgra", 3840, 2160, 1920, 1080, "uyvy", "bgra"), ("hd_same_yuyv_bgra", 1920, 1080, 1920, 1080, "yuyv", "bgra")]
    rows = []
    for frames in frame_counts:
        for point, sw, sh, src, dst in points:
            row = (sw, sh, sw, sh, src, dst, 1, 1, 1)                   # a row of tests/sws_yuy2src.py's form, not entered into its table
            c = ref.open(row)
            e = ref.describe_yuy2(c)
            ref.free(c)
            c = vref.open_formats(sw, sh, b"nv12", sw, sh, b"yuv420p", ref.flags(row))
            t = vref.describe(c)
            vref.free(c)
            assert e is not None and e.ctx.desc.unscaled_special and t is not None and t.ctx.desc.unscaled_special, point
            V.SHAPES["_bench"] = (sw, sh, sw, sh, "nv12", "420", 1, 1, 1)
            ypics = [[np.ascontiguousarray(Y.picture(row, "noise", seed=s)[0])] for s in (1, 2)]
            tpics = [[np.ascontiguousarray(pl) for pl in V.picture("_bench", seed=s)] for s in (1, 2)]
            batches = {src + "422_split": (lib, PlaneBatch(lib, Y.create(lib, e), ypics, e.out_sizes(), frames)),
                       "twin": (lib, PlaneBatch(lib, V.create(lib, t), tpics, t.out_sizes(), frames)),
                       "twin#2": (lib, PlaneBatch(lib, V.create(lib, t), tpics, t.out_sizes(), frames))}
            plan = Y.plan_of(lib, batches[src + "422_split"][1].handle)
            times = {k: [] for k in batches}
            for _ in range(a.rounds):
                for k, (l, b) in batches.items():
                    times[k].append(time_ms(l, b.run, a.steps))
            base = statistics.median(times["twin"])
            spread = abs(statistics.median(times["twin#2"]) / base - 1.0)
            twin_bytes = batches["twin"][1].src_bytes + batches["twin"][1].dst_bytes
            for k, (l, b) in batches.items():
                ms = statistics.median(times[k])
                us = ms * 1e3 / frames
                nb = b.src_bytes + b.dst_bytes
                out = {"workload": point + ":" + k, "frames_per_launch": frames, "ms_per_launch": ms, "us_per_picture": us, "frames_per_s": 1e6 / us,
                       "algorithmic_bytes_per_frame": nb, "achieved_GBps": nb / us * 1e-3, "frac_of_8TBps": nb / us * 1e-3 / 8000.0,
                       "vs_twin": ms / base - 1.0, "bound": nb / twin_bytes - 1.0, "aa_spread": spread, "ms_rounds": [round(x, 4) for x in times[k]]}
                if k not in ("twin", "twin#2"):
                    out["kernel"] = plan["kernel"]
                rows.append(out)
                print(json.dumps(out), flush=True)
            for l, b in batches.values():
                b.close()
        for point, sw, sh, dw, dh, src, dst in scaled:
            row = (sw, sh, dw, dh, src, dst, 1, 1, 1)
            c = ref.open(row)
            e = ref.describe_yuy2(c)
            ref.free(c)
            assert e is not None and not e.ctx.desc.unscaled_special, point
            t = Y.twin_entry(e)
            ypics = [[np.ascontiguousarray(Y.picture(row, "noise", seed=s)[0])] for s in (1, 2)]
            tpics = [Y.deinterleave(row, pl) for pl in ypics]

            def batch(x, pics):
                if x.fmt == 0 or x.fmt >= 32:
                    return SourceBatch(lib, None, x, pics, frames, create=Y.create, bpp=4 if x.fmt >= 33 else 3)
                return PlaneBatch(lib, Y.create(lib, x), pics, x.out_sizes(), frames)
            batches = {src + "422": (lib, batch(e, ypics)), "twin": (lib, batch(t, tpics)), "twin#2": (lib, batch(t, tpics))}
            plan = Y.plan_of(lib, batches[src + "422"][1].handle)
            times = {k: [] for k in batches}
            for _ in range(a.rounds):
                for k, (l, b) in batches.items():
                    times[k].append(time_ms(l, b.run, a.steps))
            base = statistics.median(times["twin"])
            spread = abs(statistics.median(times["twin#2"]) / base - 1.0)
            twin_bytes = batches["twin"][1].src_bytes + batches["twin"][1].dst_bytes
            for k, (l, b) in batches.items():
                ms = statistics.median(times[k])
                us = ms * 1e3 / frames
                nb = b.src_bytes + b.dst_bytes
                out = {"workload": point + ":" + k, "frames_per_launch": frames, "ms_per_launch": ms, "us_per_picture": us, "frames_per_s": 1e6 / us,
                       "algorithmic_bytes_per_frame": nb, "achieved_GBps": nb / us * 1e-3, "frac_of_8TBps": nb / us * 1e-3 / 8000.0,
                       "vs_twin": ms / base - 1.0, "bound": nb / twin_bytes - 1.0, "aa_spread": spread, "ms_rounds": [round(x, 4) for x in times[k]]}
                if k not in ("twin", "twin#2"):
                    out.update({"kernel": plan["kernel"], "hstaged": plan["hstaged"]})
                rows.append(out)
                print(json.dumps(out), flush=True)
            for l, b in batches.values():
                b.close()
    aa = max(r["aa_spread"] for r in rows)
    miss = ["%s@%d %+.1f%% (bound %+.1f%%)" % (r["workload"], r["frames_per_launch"], 100 * r["vs_twin"], 100 * (r["bound"] + aa)) for r in rows if r["vs_twin"] > r["bound"] + aa]
    print(json.dumps({"summary": "yuy2src", "aa_session": aa, "points": len(rows), "miss": miss}), flush=True)


def yuy2dst_points(a, lib, points=None, frame_counts=(32, 512), scaled=None):
    """Packed 4:2:2 destinations.  The scaler's points run beside their rgb24 twin — the context of the SAME descriptor and source to rgb24, on the same
    pictures: the same horizontal pass and the same vertical sums, two bytes a pixel written where the twin writes three and no table lookups, so
    `bound` (the ratio of algorithmic bytes) is negative: a point above its twin is a miss.  The unscaled packer (k_sws_yuy2_pack) runs beside
    k_sws_nv12_pack at the same size — the one kernel of the same kind, an interleaving copy without banks or LDS: yuv420p -> nv12 moves 3 bytes a
    pixel, yuv422p -> yuyv422 moves 4.  The contexts come from the reference's libswscale at run time (oracle/_ref/libswsref.so:
    mi355_sws_describe_yuy2dst / _src) — no full-size context is committed.  `twin#2` is the twin a second time with its own buffers: the session's A/A
    spread.  One process, the batches of a point alternating: 3 warm-up + --steps launches a round, median of --rounds rounds, at 32 and 512 pictures per
    launch.  Algorithmic bytes: the source read once + the destination written once.  The last line sums the session up: `aa_session` — the largest
    A/A spread of its points — and under `miss` every row whose time exceeds its twin's times the byte ratio plus that spread."""
    import statistics
    import numpy as np
    import sws_nv12 as N
    import sws_planar as P
    import sws_sources as X
    import sws_yuy2dst as Z
    ref = Z.Ref(P.bind(Z.REF_LIB))
    # (point, srcW, srcH, source, destination order): the packer
    points = points or [("hd_pack_yuv422p_yuyv", 1920, 1080, "yuv422p", "yuyv")]
    # (point, srcW, srcH, dstW, dstH, source, destination order): the scaler's points and the ident1 point
    scaled = scaled if scaled is not None else [("uhd_to_hd_yuv420p_yuyv", 3840, 2160, 1920, 1080, "yuv420p", "yuyv"), ("uhd_to_hd_nv12_uyvy", 3840, 2160, 1920, 1080, "nv12", "uyvy"),
                                                ("hd_same_yuv420p_yuyv", 1920, 1080, 1920, 1080, "yuv420p", "yuyv")]
    rows = []

    def report(point, frames, batches, plan, times):
        base = statistics.median(times["twin"])
        spread = abs(statistics.median(times["twin#2"]) / base - 1.0)
        twin_bytes = batches["twin"].src_bytes + batches["twin"].dst_bytes
        for k, b in batches.items():
            ms = statistics.median(times[k])
            us = ms * 1e3 / frames
            nb = b.src_bytes + b.dst_bytes
            out = {"workload": point + ":" + k, "frames_per_launch": frames, "ms_per_launch": ms, "us_per_picture": us, "frames_per_s": 1e6 / us,
                   "algorithmic_bytes_per_frame": nb, "achieved_GBps": nb / us * 1e-3, "frac_of_8TBps": nb / us * 1e-3 / 8000.0,
                   "vs_twin": ms / base - 1.0, "bound": nb / twin_bytes - 1.0, "aa_spread": spread, "ms_rounds": [round(x, 4) for x in times[k]]}
            if k not in ("twin", "twin#2"):
                out.update({"kernel": plan["kernel"], "hstaged": plan["hstaged"], "narrow": plan["narrow"]})
            rows.append(out)
            print(json.dumps(out), flush=True)

    def measure(batches):
        times = {k: [] for k in batches}
        for _ in range(a.rounds):
            for k, b in batches.items():
                times[k].append(time_ms(lib, b.run, a.steps))
        return times

    for frames in frame_counts:
        for point, sw, sh, src, dst in points:
            row = (sw, sh, sw, sh, src, 0, dst, 0, 1, 1, 1, 0)               # a row of tests/sws_yuy2dst.py's form, not entered into its table
            c = ref.open(row)
            e = ref.describe_yuy2dst(c)
            ref.free(c)
            c = ref.open_formats(sw, sh, b"yuv420p", sw, sh, b"nv12", ref.flags(row))
            t = ref.describe_src(c)
            ref.free(c)
            assert e is not None and e.ctx.desc.unscaled_special and t is not None and t.ctx.desc.unscaled_special and t.fmt == 16, point
            ypics = [[np.ascontiguousarray(pl) for pl in Z.picture(row, "noise", seed=s)] for s in (1, 2)]
            trow = (sw, sh, sw, sh, "yuv420p", 0, dst, 0, 1, 1, 1, 0)
            tpics = [[np.ascontiguousarray(pl) for pl in Z.picture(trow, "noise", seed=s)] for s in (1, 2)]
            tsizes = [(sw, sh), (2 * (sw // 2), sh // 2)]
            batches = {"pack": SourceBatch(lib, None, e, ypics, frames, create=Z.create, bpp=2),
                       "twin": PlaneBatch(lib, X.create(lib, t), tpics, tsizes, frames), "twin#2": PlaneBatch(lib, X.create(lib, t), tpics, tsizes, frames)}
            plan = Z.plan_of(lib, batches["pack"].handle)
            assert plan["kernel"] == "yuy2_pack" and N.KERNELS[9] == "nv12_pack", plan
            report(point, frames, batches, plan, measure(batches))
            for b in batches.values():
                b.close()
        for point, sw, sh, dw, dh, src, dst in scaled:
            row = (sw, sh, dw, dh, src, 0, dst, 0, 1, 1, 1, 0)
            c = ref.open(row)
            e = ref.describe_yuy2dst(c)
            ref.free(c)
            assert e is not None and not e.ctx.desc.unscaled_special and dw % 2 == 0, point
            t = Z.twin_entry(e)
            pics = [[np.ascontiguousarray(pl) for pl in Z.picture(row, "noise", seed=s)] for s in (1, 2)]
            batches = {dst + "422": SourceBatch(lib, None, e, pics, frames, create=Z.create, bpp=2),
                       "twin": SourceBatch(lib, None, t, pics, frames, create=Z.create, bpp=3), "twin#2": SourceBatch(lib, None, t, pics, frames, create=Z.create, bpp=3)}
            plan = Z.plan_of(lib, batches[dst + "422"].handle)
            report(point, frames, batches, plan, measure(batches))
            for b in batches.values():
                b.close()
    aa = max(r["aa_spread"] for r in rows)
    miss = ["%s@%d %+.1f%% (bound %+.1f%%)" % (r["workload"], r["frames_per_launch"], 100 * r["vs_twin"], 100 * (r["bound"] + aa)) for r in rows if r["vs_twin"] > r["bound"] + aa]
    print(json.dumps({"summary": "yuy2dst", "aa_session": aa, "points": len(rows), "miss": miss}), flush=True)


def p010_points(a, lib, points=None, frame_counts=(32, 512)):
    """A P010 source beside its planar 10-bit twin: the context of the SAME descriptor as a yuv420p10le source (src_layout 0, depth 10, shifts 1, 1) on
    the de-interleaved word >> 6 planes reads exactly as many source bytes and writes the same destination; the only added work is a shift and a
    permute per staged dword, so the expectation is the twin's time within the twin's own A/A spread (`bound` is 0).  The contexts come from the
    reference's libswscale at run time (oracle/_ref/libswsref.so: mi355_sws_describe_p010) — no full-size context is committed.  `twin#2` is the twin
    a second time with its own buffers: the session's A/A spread.  With --other-lib the twin also runs on that build (the parent commit's).  `copy`
    is a plain device-to-device copy of one launch's source bytes: `vs_two_step` of the P010 row is its time over the twin's plus that copy, the
    cheapest possible two-step route, which the fused path has to beat (below 0).  One process, the batches of a point alternating: 3 warm-up +
    --steps launches a round, median of --rounds rounds, at 32 and 512 pictures per launch.  Algorithmic bytes: the source planes read once + the
    destination planes written once.  The last line sums the session up: `aa_session` — the largest A/A spread of its points — and under `miss`
    every P010 row whose time exceeds its twin's by more than that spread."""
    import statistics
    import numpy as np
    import sws_planar as P
    import sws_p010 as Z
    other = None
    if a.other_lib:
        other = C.CDLL(os.path.abspath(a.other_lib))
        other.mi355_init.restype = C.c_int
        assert other.mi355_init(C.c_int(0)) == 0
        other.mi355_event_create.restype = C.c_void_p
        other.mi355_event_elapsed_ms.restype = C.c_float
    ref = Z.Ref(P.bind(Z.REF_LIB))
    # (point, srcW, srcH, dstW, dstH, destination of tests/sws_p010.py)
    points = points or [("uhd_to_hd_rgb24", 3840, 2160, 1920, 1080, "rgb24"), ("uhd_to_hd_yuv420p10le", 3840, 2160, 1920, 1080, "420p10"),
                        ("hd_same_nv12", 1920, 1080, 1920, 1080, "nv12")]
    rows = []

    def batch(l, x, pics, frames):
        if Z.one_plane(x):
            return SourceBatch(l, None, x, pics, frames, create=Z.create, bpp=4 if x.fmt >= 33 else 3)
        return PlaneBatch(l, Z.create(l, x), pics, x.out_sizes(), frames)

    for frames in frame_counts:
        for point, sw, sh, dw, dh, dst in points:
            row = (sw, sh, dw, dh, 0, dst, 0, 1, 1, 1)                  # a row of tests/sws_p010.py's form, not entered into its table
            c = ref.open(row)
            e = ref.describe_p010(c)
            ref.free(c)
            assert e is not None, point
            t = Z.twin_entry(e)
            ppics = [[np.ascontiguousarray(pl) for pl in Z.picture(row, "noise", seed=s)] for s in (1, 2)]
            tpics = [Z.planar_twin_planes(row, pic) for pic in ppics]
            batches = {"p010": (lib, batch(lib, e, ppics, frames)), "twin": (lib, batch(lib, t, tpics, frames)), "twin#2": (lib, batch(lib, t, tpics, frames))}
            if other:
                batches["twin@parent"] = (other, batch(other, t, tpics, frames))
            plan = Z.plan_of(lib, batches["p010"][1].handle)
            tplan = Z.plan_of(lib, batches["twin"][1].handle)
            # the plain copy: one launch's source bytes from one allocation to another
            nsrc = batches["p010"][1].src_bytes * frames
            lib.mi355_malloc.restype = C.c_void_p
            ca, cb = lib.mi355_malloc(C.c_size_t(nsrc)), lib.mi355_malloc(C.c_size_t(nsrc))
            assert ca and cb
            lib.mi355_memcpy_d2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
            times = {k: [] for k in batches}
            times["copy"] = []
            for _ in range(a.rounds):
                for k, (l, b) in batches.items():
                    times[k].append(time_ms(l, b.run, a.steps))
                times["copy"].append(time_ms(lib, lambda: lib.mi355_memcpy_d2d(cb, ca, nsrc), a.steps))
            lib.mi355_free(C.c_void_p(ca)); lib.mi355_free(C.c_void_p(cb))
            base = statistics.median(times["twin"])
            copy = statistics.median(times["copy"])
            spread = max(abs(x / base - 1.0) for k in ("twin#2", "twin@parent") if k in times for x in (statistics.median(times[k]),))
            twin_bytes = batches["twin"][1].src_bytes + batches["twin"][1].dst_bytes
            for k, (l, b) in batches.items():
                ms = statistics.median(times[k])
                us = ms * 1e3 / frames
                nb = b.src_bytes + b.dst_bytes
                out = {"workload": point + ":" + k, "frames_per_launch": frames, "ms_per_launch": ms, "us_per_picture": us, "frames_per_s": 1e6 / us,
                       "algorithmic_bytes_per_frame": nb, "achieved_GBps": nb / us * 1e-3, "frac_of_8TBps": nb / us * 1e-3 / 8000.0,
                       "vs_twin": ms / base - 1.0, "bound": nb / twin_bytes - 1.0, "aa_spread": spread, "ms_rounds": [round(x, 4) for x in times[k]],
                       "ms_min_max": [round(min(times[k]), 4), round(max(times[k]), 4)]}
                if k == "p010":
                    out.update({"kernel": plan["kernel"], "twin_kernel": tplan["kernel"], "hstaged": plan["hstaged"], "copy_ms": copy,
                                "vs_two_step": ms / (base + copy) - 1.0})
                rows.append(out)
                print(json.dumps(out), flush=True)
            for l, b in batches.values():
                b.close()
    aa = max(r["aa_spread"] for r in rows)
    miss = ["%s@%d %+.1f%% (spread %+.1f%%)" % (r["workload"], r["frames_per_launch"], 100 * r["vs_twin"], 100 * r["aa_spread"])
            for r in rows if r["workload"].endswith(":p010") and r["vs_twin"] > r["aa_spread"]]
    slow = ["%s@%d %+.1f%% of twin + copy" % (r["workload"], r["frames_per_launch"], 100 * r["vs_two_step"]) for r in rows if r.get("vs_two_step", -1) >= 0]
    print(json.dumps({"summary": "p010", "aa_session": aa, "points": len(rows), "miss": miss, "not_below_two_step": slow}), flush=True)


def fastbl_points(a, lib, points=None, frame_counts=(32, 512)):
    """A SWS_FAST_BILINEAR context (the bank-free horizontal pass of k_sws_fbl_generic / k_sws_fbl_planar) beside two yardsticks of the same geometry,
    source bytes and destination: `bilinear` — the reference's SWS_BILINEAR context on the bank-driven kernels (what a caller got on the device before,
    by asking for the other scaler; its vertical banks differ in size where the picture shrinks), `bilinear#2` the same a second time with its own
    buffers: the session's A/A spread; `banked` — the fast arithmetic restated as two-tap banks for the existing creator (tests/sws_fastbl.py:
    Entry.bank_twin), which for an upscale has a tap behind the line and so runs unstaged: the route the new pass replaces.  The contexts come from the
    reference's libswscale at run time (oracle/_ref/libswsref.so: mi355_sws_describe_fast and the existing describers) — no full-size context is
    committed.  One process, the batches of a point alternating: 3 warm-up + --steps launches a round, median of --rounds rounds, at 32 and 512
    pictures per launch.  Algorithmic bytes: the source planes read once + the destination planes written once.  The last line sums the session up:
    `aa_session` and, under `miss`, every fast row slower than `bilinear` by more than the point's spread."""
    import statistics
    import numpy as np
    import sws_planar as P
    import sws_fastbl as F
    ref = F.Ref(P.bind(F.REF_LIB))
    # (point, srcW, srcH, dstW, dstH, destination of tests/sws_fastbl.py)
    points = points or [("uhd_to_hd_rgb24", 3840, 2160, 1920, 1080, "rgb24"), ("uhd_to_hd_yuv420p", 3840, 2160, 1920, 1080, "420"),
                        ("hd_to_uhd_rgb24", 1920, 1080, 3840, 2160, "rgb24"), ("hd_to_uhd_yuv420p", 1920, 1080, 3840, 2160, "420")]
    rows = []

    def batch(x, pics, frames, create):
        if x.one_plane():
            return SourceBatch(lib, None, x, pics, frames, create=create, bpp=3)
        return PlaneBatch(lib, create(lib, x), pics, x.out_sizes(), frames)

    for frames in frame_counts:
        for point, sw, sh, dw, dh, dst in points:
            row = (sw, sh, dw, dh, "420", 0, dst, 0)                    # a row of tests/sws_fastbl.py's form, not entered into its table
            c = ref.open(row)
            e = ref.describe_fast(c)
            ref.free(c)
            c = ref.open(row, fast=False)
            t = ref.describe_fmt(c)
            ref.free(c)
            assert e is not None and t is not None, point
            bil = F.Entry(t.ctx, t.hsub, t.vsub, t.fmt, 0, 8, 0, 0)
            noise = F.frames(row)
            pics = [[np.ascontiguousarray(pl[:, :w]) for pl, (w, _) in zip(noise[f], F.plane_dims(row))] for f in (1, 2)]      # tightly pitched planes
            batches = {"fast": batch(e, pics, frames, F.create), "bilinear": batch(bil, pics, frames, F.create_banked),
                       "bilinear#2": batch(bil, pics, frames, F.create_banked), "banked": batch(e.bank_twin(force=True), pics, frames, F.create_banked)}
            plans = {k: F.plan_of(lib, b.handle) for k, b in batches.items()}
            times = {k: [] for k in batches}
            for _ in range(a.rounds):
                for k, b in batches.items():
                    times[k].append(time_ms(lib, b.run, a.steps))
            base, banked = statistics.median(times["bilinear"]), statistics.median(times["banked"])
            spread = abs(statistics.median(times["bilinear#2"]) / base - 1.0)
            for k, b in batches.items():
                ms = statistics.median(times[k])
                us = ms * 1e3 / frames
                nb = b.src_bytes + b.dst_bytes
                out = {"workload": point + ":" + k, "frames_per_launch": frames, "ms_per_launch": ms, "us_per_picture": us, "frames_per_s": 1e6 / us,
                       "algorithmic_bytes_per_frame": nb, "achieved_GBps": nb / us * 1e-3, "frac_of_8TBps": nb / us * 1e-3 / 8000.0,
                       "vs_bilinear": ms / base - 1.0, "vs_banked": ms / banked - 1.0, "aa_spread": spread, "kernel": plans[k]["kernel"],
                       "hstage": plans[k]["hstage"], "hstaged": plans[k]["hstaged"], "ms_rounds": [round(x, 4) for x in times[k]]}
                rows.append(out)
                print(json.dumps(out), flush=True)
            for b in batches.values():
                b.close()
    aa = max(r["aa_spread"] for r in rows)
    miss = ["%s@%d %+.1f%% (spread %+.1f%%)" % (r["workload"], r["frames_per_launch"], 100 * r["vs_bilinear"], 100 * r["aa_spread"])
            for r in rows if r["workload"].endswith(":fast") and r["vs_bilinear"] > r["aa_spread"]]
    print(json.dumps({"summary": "fast_bilinear", "aa_session": aa, "points": len(rows), "miss": miss}), flush=True)


def gbrp_points(a, lib, points=None, frame_counts=(32, 512)):
    """A gbrp destination (mi355_sws_create_gbrp: k_sws_gbrp, the arithmetic yuv -> rgb pass) from yuv420p beside two yardsticks of the same geometry and
    source bytes, both code the parent commit already had: `yuv444p` — the twin, the SAME descriptor through the existing creator to an 8-bit yuv444p
    destination (the same staging rounds, LDS and bytes written, no matrix: the difference is the new pass), `yuv444p#2` the same a second time with
    its own buffers: the session's A/A spread; `rgb24` — the reference's rgb24 context of the same sizes and flags on k_sws_generic (what a caller
    takes today, before a de-interleave of its own; the same number of bytes written, chroma at half width through the LUTs).  The contexts come from
    the reference's libswscale at run time (oracle/_ref/libswsref.so: mi355_sws_describe_gbrp and the existing describer) — no full-size context is
    committed.  One process, the batches of a point alternating: 3 warm-up + --steps launches a round, median of --rounds rounds, at 32 and 512
    pictures per launch.  Algorithmic bytes: the source planes read once + the destination planes written once.  The last line sums the session up:
    `aa_session` and, under `miss`, every gbrp row slower than its twin by more than the point's spread."""
    import statistics
    import numpy as np
    import sws_planar as P
    import sws_fastbl as F
    import sws_gbrp as B
    ref = B.Ref(P.bind(B.REF_LIB))
    points = points or [("uhd_to_hd", 3840, 2160, 1920, 1080), ("hd_to_uhd", 1920, 1080, 3840, 2160), ("hd_to_360p", 1920, 1080, 640, 360)]
    rows = []
    for frames in frame_counts:
        for point, sw, sh, dw, dh in points:
            row = (sw, sh, dw, dh, "yuv420p", 1, 0, None)               # a row of tests/sws_gbrp.py's form, not entered into its table
            c = ref.open(row)
            e = ref.describe_gbrp(c)
            ref.free(c)
            c = ref.open(row, dst=b"rgb24")
            t = ref.describe_fmt(c)
            ref.free(c)
            assert e is not None and t is not None, point
            rgb = F.Entry(t.ctx, t.hsub, t.vsub, t.fmt, 0, 8, 0, 0)
            noise = B.frames(row)
            pics = [[np.ascontiguousarray(pl[:, :w]) for pl, (w, _) in zip(noise[f], F.plane_dims((sw, sh, dw, dh, "420", 0, "444", 0)))] for f in (0, 2)]      # tightly pitched planes
            batches = {"gbrp": PlaneBatch(lib, B.create(lib, e), pics, e.out_sizes(), frames),
                       "yuv444p": PlaneBatch(lib, B.create_twin(lib, e), pics, e.out_sizes(), frames),
                       "yuv444p#2": PlaneBatch(lib, B.create_twin(lib, e), pics, e.out_sizes(), frames),
                       "rgb24": SourceBatch(lib, None, rgb, pics, frames, create=F.create_banked, bpp=3)}
            plans = {k: F.plan_of(lib, b.handle) for k, b in batches.items()}
            times = {k: [] for k in batches}
            for _ in range(a.rounds):
                for k, b in batches.items():
                    times[k].append(time_ms(lib, b.run, a.steps))
            base, packed = statistics.median(times["yuv444p"]), statistics.median(times["rgb24"])
            spread = abs(statistics.median(times["yuv444p#2"]) / base - 1.0)
            for k, b in batches.items():
                ms = statistics.median(times[k])
                us = ms * 1e3 / frames
                nb = b.src_bytes + b.dst_bytes
                out = {"workload": point + ":" + k, "frames_per_launch": frames, "ms_per_launch": ms, "us_per_picture": us, "frames_per_s": 1e6 / us,
                       "algorithmic_bytes_per_frame": nb, "achieved_GBps": nb / us * 1e-3, "frac_of_8TBps": nb / us * 1e-3 / 8000.0,
                       "vs_yuv444p": ms / base - 1.0, "vs_rgb24": ms / packed - 1.0, "aa_spread": spread, "kernel": plans[k]["kernel"],
                       "hstage": plans[k]["hstage"], "hstaged": plans[k]["hstaged"], "ms_rounds": [round(x, 4) for x in times[k]]}
                rows.append(out)
                print(json.dumps(out), flush=True)
            for b in batches.values():
                b.close()
    aa = max(r["aa_spread"] for r in rows)
    miss = ["%s@%d %+.1f%% (spread %+.1f%%)" % (r["workload"], r["frames_per_launch"], 100 * r["vs_yuv444p"], 100 * r["aa_spread"])
            for r in rows if r["workload"].endswith(":gbrp") and r["vs_yuv444p"] > r["aa_spread"]]
    print(json.dumps({"summary": "gbrp", "aa_session": aa, "points": len(rows), "miss": miss}), flush=True)


if __name__ == "__main__":
    main()
