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
    ap.add_argument("--rounds", type=int, default=5, help="--planar: alternating rounds (the median is reported)")
    a = ap.parse_args()
    prov = providers.mi355()
    lib = prov.lib
    lib.mi355_event_create.restype = C.c_void_p
    lib.mi355_event_elapsed_ms.restype = C.c_float
    if a.planar:
        return planar(a, lib)
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


if __name__ == "__main__":
    main()
