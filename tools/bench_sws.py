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
    ap.add_argument("--rounds", type=int, default=5, help="--planar / --sources: alternating rounds (the median is reported)")
    a = ap.parse_args()
    prov = providers.mi355()
    lib = prov.lib
    lib.mi355_event_create.restype = C.c_void_p
    lib.mi355_event_elapsed_ms.restype = C.c_float
    if a.planar:
        return planar(a, lib)
    if a.sources:
        return sources(a, lib)
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

    def __init__(self, lib, X, e, pics, frames):
        self.lib, self.bufs, self.n = lib, [], frames
        lib.mi355_malloc.restype = C.c_void_p
        lib.mi355_malloc.argtypes = [C.c_size_t]
        lib.mi355_free.argtypes = [C.c_void_p]
        for f in ("mi355_memcpy_h2d", "mi355_memcpy_d2d"):
            getattr(lib, f).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        d = e.ctx.desc
        arr = (S.SwsFrame * frames)()
        self.src_bytes = 0
        for p in range(3):
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
        self.dst_bytes = d.dstW * 3 * d.dstH
        dst = self.alloc(frames * self.dst_bytes + 64)
        for f in range(frames):
            arr[f].dst, arr[f].dst_stride = dst + f * self.dst_bytes, d.dstW * 3
        self.d_frames = self.alloc(C.sizeof(arr))
        lib.mi355_memcpy_h2d(self.d_frames, C.addressof(arr), C.sizeof(arr))
        self.handle = X.create(lib, e)
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


if __name__ == "__main__":
    main()
