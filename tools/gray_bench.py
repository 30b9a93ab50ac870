#!/usr/bin/env python3
"""Development helper (GPU box): device-resident throughput of the gray mode (MI355_F_GRAY) against standard 4:2:0,
timed the same way in the same process.  128 x 3840x2160 LCG frames per call at q50 (gray: synth_lcg_device with
frame_bytes = W*H; 4:2:0: W*H*3), then one frame per call (latency).  Prints one JSON line per case and a summary line
with the gray / 4:2:0 ratio.

    python tools/gray_bench.py [--frames 128] [--reps 10]"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
jpeg = importlib.import_module("jpeg-encoder-opencl_amd")
import torch  # noqa: E402

W, H, CAP = 3840, 2160, 8 << 20


def run(name, comps, flags, n, reps, warmup=2):
    enc = jpeg.Encoder(0)
    enc.set_quality(50)
    dev = torch.device("cuda", 0)
    d_in = torch.empty(n * W * H * comps, dtype=torch.uint8, device=dev)
    enc.synth_lcg_device(d_in.data_ptr(), W * H * comps, n, 1)
    d_out = torch.zeros((n, CAP), dtype=torch.uint8, device=dev)
    d_bits = torch.zeros(n, dtype=torch.int64, device=dev)

    def go():
        enc.encode_scan_device(d_in.data_ptr(), W, H, n, d_out.data_ptr(), CAP, d_bits.data_ptr(), flags=flags)

    for _ in range(warmup):
        go()
    enc.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        go()
    enc.sync()
    dt = (time.perf_counter() - t0) / reps
    bits = d_bits.cpu().numpy()
    rec = {"case": name, "frames": n, "W": W, "H": H, "quality": 50, "flags": flags, "parts": enc.last_call_parts(),
           "ms_per_call": round(dt * 1e3, 4), "Gpixel_per_s": round(n * W * H / dt / 1e9, 2),
           "bits_per_pixel": round(float(bits.sum()) / (n * W * H), 3)}
    print(json.dumps(rec), flush=True)
    enc.close()
    del d_in, d_out, d_bits
    torch.cuda.empty_cache()
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    gray = run("gray 4K q50", 1, jpeg.F_STANDARD | jpeg.F_GRAY, a.frames, a.reps)
    s420 = run("standard 4:2:0 4K q50", 3, jpeg.F_STANDARD | jpeg.F_420, a.frames, a.reps)
    g1 = run("gray 4K q50, one frame per call", 1, jpeg.F_STANDARD | jpeg.F_GRAY, 1, 50)
    s1 = run("standard 4:2:0 4K q50, one frame per call", 3, jpeg.F_STANDARD | jpeg.F_420, 1, 50)
    print(json.dumps({"summary": "gray vs 4:2:0", "gray_Gpixel_per_s": gray["Gpixel_per_s"],
                      "s420_Gpixel_per_s": s420["Gpixel_per_s"],
                      "ratio": round(gray["Gpixel_per_s"] / s420["Gpixel_per_s"], 3),
                      "gray_latency_ms": g1["ms_per_call"], "s420_latency_ms": s1["ms_per_call"],
                      "torch": torch.__version__, "hip": torch.version.hip}), flush=True)
