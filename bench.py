#!/usr/bin/env python3
"""Headline benchmark: Mpixels/s of the strict JPEG encode path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR]

Workload (BASELINE.json configs[1], batched so that the timed region is long enough to mean
something): one step = ONE call of mi355_jpeg_encode_scan_device on a batch of
`--frames-per-step` (default 128) distinct synthetic 3840x2160 RGB frames (LCG noise, seed =
1 + global frame index), q=50 tables, chroma averaging on, strict (bit-exact)
mode, device-resident RGB in -> device-resident packed scan bits out, on one HIP stream.  The
frames are generated in HBM before the timed region; every step encodes the same resident batch.

Multi-GPU: one process per GPU.  `python bench.py --gpus N` starts its own N worker processes
(before anything touches a GPU); under torchrun (RANK/WORLD_SIZE in the environment) it is a
worker itself.  torch.distributed (backend nccl = RCCL) carries the barrier and the
max-over-ranks only: frames are independent, so ranks shard the frames with no data-path
collective -- "scaling": "weak" (every rank encodes K x frames-per-step frames).

Prints ONE JSON line on rank 0:
  roofline      the dominant kernel (k_screen_encode: fused colour conversion, integer-MFMA
                transform, quantise+verify, per-unit RLE/Huffman), timed with HIP events on its
                launch stream INSIDE the timed region (the library brackets the kernel launches
                of every call; a bracket spans the call's launches back to back);
  cpu_baseline  the reference CPU path (oracle/_ref, built from the reference's own sources) or,
                where that is not loadable, the C restatement, one host core, one frame -- on rank 0
                after the timed region, at every N (north_star: "next to the reference's own CPU
                path ... in the same run");
  end_to_end    secondary: pinned host RGB -> host scan bytes through mi355_jpeg_pool_encode over
                ALL the run's GPUs (PCIe both ways; Gpixel/s and H2D GB/s per GPU) -- never `value`;
  standard_mode secondary: the decodable 4:2:0 baseline mode (not a behaviour of the reference);
  single_call_latency_ms   one 4K frame per call, one call at a time.
  other_configs the other BASELINE configurations and SURVEY §8(d)'s natural-statistics input, each gated on a golden
                of the reference build first (tests/golden/cases.json; 16384^2: SURVEY Appendix B), each with Mpixel/s,
                algorithmic GB/s and fraction of the HBM roof by §8(d)'s formula: configs[2] (256 x 1080p q75 per call),
                configs[4] (one 16384x16384 q90 frame without chroma averaging), fruit.ppm tiled to 3840x2160 in strict
                mode and in standard 4:2:0 -- secondary, never `value`.
All outputs written in the timed region are re-verified after it (see verify_outputs).
--dump-outputs DIR also writes what the last timed step computed as .npy files (see dump_outputs).
"""
import argparse
import hashlib
import importlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

W, H, QUALITY = 3840, 2160, 50
FBYTES = W * H * 3
GOLDEN_SEED1_BITS = 38227880
GOLDEN_SEED1_SHA = "6a4a20a6412d6e3bfd878e09875156170ff80a74d7c10c04b52a425e7dbcf009"
HBM_PEAK_GBPS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
ALG_FP64_OPS_PER_UNIT = 12416   # 64*64*3 + 64 + 64 per (block, channel)
DTYPE = "i8-mfma + fp32 screen, f64 arbiter (results bit-identical to the reference's f64 path)"
GOLDEN_16K = (3938207090, "22a3a76e3a7ceb82d483d31262f3b67bce5668bed019bcca7f457094bb64fe54")  # 16384^2 LCG seed 1, q90, no averaging


def golden_4k():
    """{seed: (bits, sha256)} of 4K LCG frames at q50 with chroma averaging, from the reference build
    (tests/golden/cases.json, written by tools/make_golden.py)."""
    out = {1: (GOLDEN_SEED1_BITS, GOLDEN_SEED1_SHA)}
    try:
        for c in json.load(open(os.path.join(ROOT, "tests", "golden", "cases.json"))):
            if c.get("W") == W and c.get("H") == H and c.get("quality") == QUALITY and c.get("cds_on") and \
                    c["name"].startswith("lcg_") and "seed" in c:
                out[int(c["seed"])] = (int(c["n_bits"]), c["sha256_ascii_bits"])
    except Exception:
        pass
    return out


def golden_case(name):
    try:
        for c in json.load(open(os.path.join(ROOT, "tests", "golden", "cases.json"))):
            if c["name"] == name:
                return c
    except Exception:
        pass
    return None


def gate_other_quality(enc, torch, dev):
    """Pre-region parity gate on a second operating point: one 2048x2048 LCG frame at q=90 WITHOUT chroma averaging
    against the reference build's golden (tests/golden/cases.json).  A timing variant that is only wrong away from
    q50 / 4K (one was, round 2) fails here instead of passing the q50 gate.  Returns the case name or None."""
    c = golden_case("lcg_2048x2048_s1_q90_nocds")
    if c is None:
        return None
    w, h = c["W"], c["H"]
    d = torch.empty((1, h, w, 3), dtype=torch.uint8, device=dev)
    enc.synth_lcg_device(d.data_ptr(), w * h * 3, 1, c["seed"])
    cap = ((c["n_bits"] + 7) // 8 + 4096) & ~3
    o = torch.zeros((1, cap), dtype=torch.uint8, device=dev)
    b = torch.zeros(1, dtype=torch.int64, device=dev)
    enc.set_quality(c["quality"])
    try:
        enc.encode_scan_device(d.data_ptr(), w, h, 1, o.data_ptr(), cap, b.data_ptr(), flags=0)
        enc.sync()
    finally:
        enc.set_quality(QUALITY)
    nb = int(b[0])
    assert nb == c["n_bits"], "q90 gate: %d bits, reference %d" % (nb, c["n_bits"])
    assert ascii_sha(o[0, :(nb + 7) // 8].cpu().numpy(), nb) == c["sha256_ascii_bits"], "q90 gate: scan bits differ from the reference"
    return c["name"]


def ascii_sha_chunked(packed_torch_u8, nb, chunk=16 << 20):
    """ascii_sha of a long scan without holding its 8-fold expansion: the packed bytes come from the device in pieces."""
    h = hashlib.sha256()
    nbytes = (nb + 7) // 8
    for lo in range(0, nbytes, chunk):
        hi = min(lo + chunk, nbytes)
        bits = np.unpackbits(packed_torch_u8[lo:hi].cpu().numpy())
        if hi == nbytes:
            bits = bits[:nb - lo * 8]
        h.update((bits + ord("0")).astype(np.uint8).tobytes())
    return h.hexdigest()


def tiled_fruit(w, h):
    """SURVEY §8(d)'s natural-statistics input: src[(y mod 254) * 253 + (x mod 253)] of the reference's data/fruit.ppm
    (tests/golden/fruit.ppm is that file)."""
    with open(os.path.join(ROOT, "tests", "golden", "fruit.ppm"), "rb") as f:
        assert f.readline().strip() == b"P6"
        fw, fh = (int(v) for v in f.readline().split())
        assert int(f.readline()) == 255
        fruit = np.frombuffer(f.read(fw * fh * 3), np.uint8).reshape(fh, fw, 3)
    return np.ascontiguousarray(fruit[np.arange(h) % fh][:, np.arange(w) % fw])


def other_configs_leg(jpeg, enc, torch, dev, stream):
    """The BASELINE configurations besides the headline one and SURVEY §8(d)'s natural input, device-resident, one call
    shape each, gated on a golden before it is timed.  Algorithmic bytes per frame = 3 W H + ceil(bits / 8)."""
    out = []

    def run(name, w, h, n, quality, flags, fill, gate, reps, note):
        enc.set_quality(quality)
        d = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
        fill(d)
        enc.sync()
        cap = gate["cap"]
        o = torch.zeros((n, cap), dtype=torch.uint8, device=dev)
        b = torch.zeros(n, dtype=torch.int64, device=dev)

        def go():
            enc.encode_scan_device(d.data_ptr(), w, h, n, o.data_ptr(), cap, b.data_ptr(), flags=flags, stream=stream)

        go()
        enc.sync(stream)
        nb0 = int(b[0])
        assert nb0 == gate["n_bits"], "%s: frame 0 has %d bits, golden %d" % (name, nb0, gate["n_bits"])
        if "sha_ascii" in gate:
            assert ascii_sha_chunked(o[0], nb0) == gate["sha_ascii"], "%s: scan bits differ from the reference" % name
        else:
            assert hashlib.sha256(o[0, :(nb0 + 7) // 8].cpu().numpy().tobytes()).hexdigest() == gate["sha_packed"], \
                "%s: scan bytes differ from the checker's fixture" % name
        # warm-up: a new shape gives the library a new workspace, and the first calls after one (and after the host-side
        # input generation above) run up to 8 % slower than the steady state (tools/uneven_probe.py: 3.53, 3.42, 3.34, 3.30,
        # 3.25 ms for the first five 100-frame calls of a context) -- the headline leg has its --warmup steps for the same reason
        tw = time.perf_counter()
        while time.perf_counter() - tw < 0.04:
            go()
            enc.sync(stream)
        enc.walk_stats(reset=True)
        enc.set_profiling(2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            go()
        enc.sync(stream)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        prof, calls = enc.profile_summary()
        enc.set_profiling(0)
        rewalked, general = enc.walk_stats(reset=True)
        bits = b.cpu().numpy().astype(np.int64)
        assert (bits > 0).all() and (bits <= 8 * cap).all(), name
        alg = 3.0 * w * h + float(np.mean((bits + 7) // 8))
        gbps = alg * n / dt / 1e9
        t_k = prof["transform_ms"] / max(calls, 1) * 1e-3
        units = n * (-(-w // 8)) * (-(-h // 8)) * 3
        rec = {"case": name, "value": round(n * w * h / dt / 1e6, 1), "unit": "Mpixel/s", "frames_per_call": n, "ms_per_call": round(dt * 1e3, 4),
               "bits_per_pixel": round(float(bits.mean()) / (w * h), 4), "algorithmic_bytes_per_frame": int(alg),
               "achieved_GBps": round(gbps, 1), "frac_of_hbm_peak": round(gbps / HBM_PEAK_GBPS, 5),
               "block_encode_kernel_ms_per_call": round(t_k * 1e3, 4), "block_encode_kernel_GBps": round(alg * n / t_k / 1e9, 1),
               "gated_on": gate["what"], "note": note}
        if not (flags & jpeg.F_STANDARD):
            rec["strings_walked_twice_per_unit"] = round(rewalked / float(reps * units), 4)
            rec["passes_in_general_walk_loop"] = round(general / float(reps * units / 64.0), 4)
        out.append(rec)
        del d, o, b
        torch.cuda.empty_cache()

    def lcg(seed0):
        return lambda d: enc.synth_lcg_device(d.data_ptr(), d.shape[1] * d.shape[2] * 3, d.shape[0], seed0)

    def fruit(d):
        f = torch.from_numpy(tiled_fruit(d.shape[2], d.shape[1])).to(d.device)
        d[:] = f

    try:
        c = golden_case("lcg_1920x1080_s1_q75_cds")
        run("configs[2]: 256 x 1920x1080 LCG frames per call (of the 1024), q75, chroma averaging on, strict", 1920, 1080, 256, 75,
            jpeg.F_DEFAULT, lcg(1), {"n_bits": c["n_bits"], "sha_ascii": c["sha256_ascii_bits"], "cap": 3 << 20,
                                     "what": "tests/golden/cases.json lcg_1920x1080_s1_q75_cds (reference build)"}, 4,
            "Huffman prefix-scan throughput (BASELINE)")
        run("configs[4]: one 16384x16384 LCG frame, q90, no chroma averaging, strict", 16384, 16384, 1, 90, 0, lcg(1),
            {"n_bits": GOLDEN_16K[0], "sha_ascii": GOLDEN_16K[1], "cap": 520 << 20, "what": "SURVEY Appendix B (reference build): 3 938 207 090 bits, 22a3a76e..."},
            4, "DCT/quant HBM-roofline stress (BASELINE): 14.7 bit/px; values beyond the whole-symbol table in nearly every pass "
               "(passes_in_general_walk_loop), no string beyond its 24-word LDS slot (strings_walked_twice_per_unit)")
        c = golden_case("lcg_3840x2160_s1_q50_cds")
        run("the headline workload at 100 frames per call (a batch size other than the tuned one)", W, H, 100, 50, jpeg.F_DEFAULT, lcg(1),
            {"n_bits": c["n_bits"], "sha_ascii": c["sha256_ascii_bits"], "cap": 8 << 20, "what": "tests/golden/cases.json lcg_3840x2160_s1_q50_cds (reference build)"},
            6, "until round 4 (one k_merge workgroup per CU, equal parts) a batch that did not divide evenly lost 8 %: a part's merge "
               "outlasted the block encode it ran beside and the next launch's persistent workgroups waited for LDS (DESIGN.md 4.5)")
        c = golden_case("fruit_tiled_3840x2160_q50_cds")
        run("natural statistics, strict: fruit.ppm tiled to 3840x2160, 128 frames per call, q50, chroma averaging on", W, H, 128, 50,
            jpeg.F_DEFAULT, fruit, {"n_bits": c["n_bits"], "sha_ascii": c["sha256_ascii_bits"], "cap": 8 << 20,
                                    "what": "tests/golden/cases.json fruit_tiled_3840x2160_q50_cds (reference build; SURVEY Appendix B a23fc925...)"}, 4,
            "SURVEY §8(d)'s secondary input; the reference's in-place chain is not a DCT, so even a photograph keeps 4.7 bit/px here")
        c = golden_case("std420_fruit_tiled_3840x2160_q50")
        run("natural statistics, standard 4:2:0: fruit.ppm tiled to 3840x2160, 128 frames per call, q50", W, H, 128, 50,
            jpeg.F_STANDARD | jpeg.F_420, fruit, {"n_bits": c["n_bits"], "sha_packed": c["sha256_packed_bits"], "cap": 4 << 20,
                                                 "what": "tests/golden/cases.json std420_fruit_tiled_3840x2160_q50 (the checker's fixture: this mode is not a behaviour of the reference)"},
            6, "the decodable mode on a photograph: 1.6 bit/px, a third of the symbols of noise")
    finally:
        enc.set_quality(QUALITY)
    return out


def kernel_sources_sha():
    """Identifies the kernel sources -- and the Makefile with the compiler flags -- a PMC measurement belongs to (the GPU box
    has no .git)."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "jpeg-encoder-opencl_amd", "csrc")
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".h", ".cpp")):
            h.update(name.encode())
            h.update(open(os.path.join(d, name), "rb").read())
    h.update(b"Makefile")
    h.update(open(os.path.join(ROOT, "jpeg-encoder-opencl_amd", "Makefile"), "rb").read())
    return h.hexdigest()[:16]


def lcg_frames(n, seed0, w, h):
    """uint8 [n, h, w, 3]; s <- s*1664525 + 1013904223 (mod 2^32), byte = s >> 24, seed = seed0 + f.
    Vectorised by jumping ahead: s_k = A_k*s0 + C_k."""
    m = w * h * 3
    a = np.empty(m, np.uint32)
    c = np.empty(m, np.uint32)
    A, Cc = np.uint32(1664525), np.uint32(1013904223)
    a[0], c[0] = A, Cc
    filled = 1
    with np.errstate(over="ignore"):
        while filled < m:
            n2 = min(filled, m - filled)
            a[filled:filled + n2] = a[:n2] * a[filled - 1]
            c[filled:filled + n2] = c[:n2] * a[filled - 1] + c[filled - 1]
            filled += n2
        out = np.empty((n, m), np.uint8)
        for f in range(n):
            s = a * np.uint32(seed0 + f) + c
            out[f] = (s >> np.uint32(24)).astype(np.uint8)
    return out.reshape(n, h, w, 3)


def shard_seed0(rank, frames):
    """Frames are sharded across ranks with no overlap: rank r owns LCG seeds
    1 + r*frames ... (r+1)*frames (seed = 1 + global frame index)."""
    return 1 + rank * frames


def ascii_sha(packed, nb):
    """SHA-256 of the '0'/'1' string the reference's HuffmanEncoder returns (utils.cpp:697)."""
    return hashlib.sha256((np.unpackbits(packed)[:nb] + ord("0")).astype(np.uint8).tobytes()).hexdigest()


DUMP_SAMPLE_SEED = 1234
DUMP_BUDGET_BYTES = 48 << 20  # all ranks together; --dump-outputs promises at most 64 MB


def dump_outputs(dirname, out, n_bits, rank, world):
    """--dump-outputs: what the last timed step handed its caller -- every frame's scan bit count and its packed scan
    bytes (`out` [frames, cap] uint8, torch, any device) -- as .npy files in float64 / float32.  The packed buffer is far
    over the size limit, so its bytes go as a fixed sample: the same seeded positions in every frame slot, with the bytes
    past a frame's scan and the unused low bits of its last byte written as 0.  Files are prefixed rankN_ when N > 1."""
    import torch
    os.makedirs(dirname, exist_ok=True)
    F, cap = out.shape
    nb = np.asarray(n_bits, np.int64)
    per_frame = max(1, min(cap, DUMP_BUDGET_BYTES // 4 // (F * world)))
    pos = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(cap, per_frame, replace=False))
    sample = out[:, torch.from_numpy(pos).to(out.device)].cpu().numpy().astype(np.int64)
    nbytes = (nb + 7) // 8
    sample[pos[None, :] >= nbytes[:, None]] = 0
    last = pos[None, :] == nbytes[:, None] - 1
    keep = (0xFF << ((8 - nb % 8) % 8)) & 0xFF  # bits of the last byte that belong to the scan
    sample = np.where(last, sample & keep[:, None], sample)
    pre = "rank%d_" % rank if world > 1 else ""
    np.save(os.path.join(dirname, pre + "scan_n_bits.npy"), nb.astype(np.float64))
    np.save(os.path.join(dirname, pre + "scan_bytes_sample.npy"), sample.astype(np.float32))
    np.save(os.path.join(dirname, pre + "scan_bytes_sample_index.npy"), pos.astype(np.float64))


# ---------------------------------------------------------------------------------------------
# process layout
# ---------------------------------------------------------------------------------------------
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_workers(args, argv):
    """`python bench.py --gpus N` without a launcher: N fresh worker processes, one per GPU, started
    before this process has touched any GPU (it never does).  Rank 0 prints the JSON line on the
    shared stdout; the exit code is the first non-zero one."""
    port = free_port()
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), MI355_BENCH_SPAWNED="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env))
    rc = 0
    deadline = time.time() + args.worker_timeout
    alive = list(procs)
    while alive:
        for p in list(alive):
            r = p.poll()
            if r is not None:
                alive.remove(p)
                if r != 0 and rc == 0:
                    rc = r
                    deadline = min(deadline, time.time() + args.dead_rank_grace)  # a rank died: the others cannot finish
        if alive and time.time() > deadline:
            for p in alive:  # exactly the processes started above
                p.kill()
            rc = rc or 124
            break
        time.sleep(0.05)
    return rc


def dist_env():
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    return rank, local_rank, world


def timed_region(step, steps, dist, distributed, sync):
    """Barrier + device sync on both sides of exactly `steps` steps."""
    if distributed:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for i in range(steps):
        step(i)
    sync()
    if distributed:
        dist.barrier()
    return time.perf_counter() - t0


def gather_times(dt, dist, distributed, device):
    """(max over ranks, [per-rank seconds])."""
    if not distributed:
        return dt, [dt]
    import torch
    t = torch.tensor([dt], dtype=torch.float64, device=device)
    allt = [torch.zeros_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(allt, t)
    per = [float(x.item()) for x in allt]
    return max(per), per


# ---------------------------------------------------------------------------------------------
# CPU rehearsal of the multi-process path (tests only)
# ---------------------------------------------------------------------------------------------
def dry_run_cpu(args):
    """TEST-ONLY rehearsal of the multi-process path on CPU (gloo): same launcher, sharding, barrier,
    timing and aggregation code as the GPU run, with the oracle standing in as the worker on
    tiny frames.  Used by tests/test_bench_distributed.py; never a benchmark result."""
    import torch
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as ol
    rank, _, world = dist_env()
    distributed = world > 1
    if os.environ.get("MI355_BENCH_TEST_FAIL_RANK") == str(rank):  # tests: a rank that dies before the rendezvous
        sys.exit(3)
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="gloo")
    assert world == args.gpus
    w, h, F = 64, 48, max(1, args.frames_per_step)
    frames = lcg_frames(F, shard_seed0(rank, F), w, h)
    bits = [0] * F
    scans = [None] * F

    def step(i):
        for k in range(F):
            o = ol.oracle_encode(frames[k])
            bits[k], scans[k] = o.n_bits, o.bits

    for i in range(args.warmup):
        step(i)
    dt = timed_region(step, args.steps, dist, distributed, lambda: None)
    dt, per = gather_times(dt, dist, distributed, "cpu")
    if args.dump_outputs:
        out = torch.zeros((F, max(len(b) for b in scans)), dtype=torch.uint8)
        for k, b in enumerate(scans):
            out[k, :len(b)] = torch.from_numpy(np.asarray(b, np.uint8))
        dump_outputs(args.dump_outputs, out, bits, rank, world)
    allbits = [None] * world
    if distributed:
        dist.all_gather_object(allbits, bits)
    else:
        allbits = [bits]
    if rank == 0:
        # the same secondary keys the GPU run carries at every N, with the oracle standing in (tests assert their presence)
        t0 = time.perf_counter()
        nb = ol.oracle_encode(frames[0]).n_bits
        t1 = time.perf_counter() - t0
        secondary = {"cpu_baseline": {"value": round(w * h / t1 / 1e6, 4), "unit": "Mpixel/s", "cores": 1, "kind": "port",
                                      "sample": "dry run: one %dx%d frame, %d bits" % (w, h, nb)},
                     "end_to_end": {"value": None, "unit": "Mpixel/s", "gpus": world, "note": "dry run: no device"}}
        print(json.dumps({"metric": "DRY RUN (cpu oracle, gloo) -- not a benchmark", "n_gpus": world, **secondary,
                          "ranks_seen": dist.get_world_size() if distributed else 1,
                          "launcher": "bench.py" if os.environ.get("MI355_BENCH_SPAWNED") else "external",
                          "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 5),
                          "scaling": "weak", "value": round(world * args.steps * F * w * h / dt / 1e6, 4), "unit": "Mpixel/s",
                          "per_rank_mpixel_s": [round(args.steps * F * w * h / t / 1e6, 4) for t in per],
                          "seed0_per_rank": [shard_seed0(r, F) for r in range(world)],
                          "bits_per_rank": allbits}), flush=True)
    if distributed:
        dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------
# CPU baseline (the checker's leg: oracle/_ref or the C restatement)
# ---------------------------------------------------------------------------------------------
def cpu_baseline():
    """Reference CPU path on ONE 4K frame (seed 1), one host thread."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as ol
    rgb = ol.lcg_frame(W, H, 1)
    ql, qc = ol.quant_tables(QUALITY)
    kind = "reference" if ol.ref() is not None else "port"
    t0 = time.perf_counter()
    r = ol.ref_encode(rgb, ql, qc, True) if kind == "reference" else ol.oracle_encode(rgb, ql, qc, True)
    dt = time.perf_counter() - t0
    assert r.n_bits == GOLDEN_SEED1_BITS
    stage = r.stage_us
    return {
        "value": round(W * H / dt / 1e6, 4), "unit": "Mpixel/s", "cores": 1, "kind": kind,
        "sample": "1 frame 3840x2160 LCG seed 1, q50, chroma averaging on, whole CPU path "
                  "(CSC..Huffman string), %.2f s wall, transform stage %.2f s" % (dt, stage[4] / 1e6),
    }, r


def cpu_baseline_multicore(max_threads=16):
    """The generous version of the CPU baseline: one 4K frame per host thread, all threads at
    once (the reference itself is single-threaded; ctypes releases the GIL inside the C call)."""
    import concurrent.futures
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as ol
    n = max(1, min(max_threads, os.cpu_count() or 1))
    rgb = ol.lcg_frame(W, H, 1)
    ql, qc = ol.quant_tables(QUALITY)
    use_ref = ol.ref() is not None
    fn = (lambda: ol.ref_encode(rgb, ql, qc, True).n_bits) if use_ref else (lambda: ol.oracle_encode(rgb, ql, qc, True).n_bits)
    t0 = time.perf_counter()
    with concurrent.futures.ThreadPoolExecutor(n) as ex:
        bits = list(ex.map(lambda _: fn(), range(n)))
    dt = time.perf_counter() - t0
    assert all(b == GOLDEN_SEED1_BITS for b in bits)
    return {"value": round(n * W * H / dt / 1e6, 4), "unit": "Mpixel/s", "cores": n,
            "kind": "reference" if use_ref else "port",
            "sample": "%d frames 3840x2160 (LCG seed 1), one per host thread, %.2f s wall" % (n, dt)}


# ---------------------------------------------------------------------------------------------
# the GPU worker
# ---------------------------------------------------------------------------------------------
def worker(args):
    import torch
    import torch.distributed as dist

    rank, local_rank, world = dist_env()
    distributed = world > 1 or args.rehearse_dist
    assert world == args.gpus, "WORLD_SIZE=%d but --gpus %d" % (world, args.gpus)
    if args.rehearse_dist and world == 1:  # the process-group path (RCCL init, barrier, all_gather, gloo tail group) with one rank
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        os.environ.setdefault("MASTER_PORT", str(free_port()))
    ndev = torch.cuda.device_count()
    device_index = local_rank if not args.share_device else local_rank % max(ndev, 1)
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", device_index))
        else:  # rehearsal of the multi-process GPU path on a box with fewer GPUs than ranks
            dist.init_process_group(backend="gloo")
    torch.cuda.set_device(device_index)
    dev = torch.device("cuda", device_index)
    coll_dev = dev if args.backend == "nccl" else "cpu"
    # the other ranks wait for rank 0's CPU baseline / end-to-end leg on the CPU, not inside a spinning RCCL kernel
    tail_group = dist.new_group(backend="gloo") if distributed and args.backend == "nccl" else None

    jpeg = importlib.import_module("jpeg-encoder-opencl_amd")
    enc = jpeg.Encoder(device_index)
    enc.set_quality(QUALITY)

    F = max(1, args.frames_per_step)
    seed0 = shard_seed0(rank, F)
    # the resident batch of pinned LCG frames is generated in place on the device (the parity gates
    # below check rank 0's frames against the reference's golden SHA-256s)
    d_rgb = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    enc.synth_lcg_device(d_rgb.data_ptr(), FBYTES, F, seed0)
    enc.sync()
    cap = args.cap_mb << 20  # bytes per frame slot (noise at q50 needs 4.8 MB)
    d_out = torch.zeros((F, cap), dtype=torch.uint8, device=dev)
    d_bits = torch.zeros(F, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def step(_i):
        enc.encode_scan_device(d_rgb.data_ptr(), W, H, F, d_out.data_ptr(), cap, d_bits.data_ptr(), stream=stream)

    def sync():
        enc.sync(stream)
        torch.cuda.synchronize()

    golden = golden_4k()

    def verify_outputs(tag, ref_bits=None, ref_out=None):
        """Bit counts of every frame of the batch, SHA-256 against the reference build's goldens for the
        frames that have one (rank 0 owns seed 1...), and -- after the timed region -- byte equality of
        every output with the copy taken from the isolated pre-region call."""
        bits = d_bits.cpu().numpy().astype(np.int64)
        assert (bits > 0).all() and (bits <= 8 * cap).all(), "%s: implausible bit counts" % tag
        checked = 0
        for k in range(F):
            g = golden.get(seed0 + k)
            if g is None or checked >= args.verify_frames:
                continue
            nb = int(bits[k])
            assert nb == g[0], "%s: frame seed %d: %d bits, reference %d" % (tag, seed0 + k, nb, g[0])
            sha = ascii_sha(d_out[k, :(nb + 7) // 8].cpu().numpy(), nb)
            assert sha == g[1], "%s: frame seed %d: scan bits differ from the reference" % (tag, seed0 + k)
            checked += 1
        if ref_bits is not None:
            assert np.array_equal(bits, ref_bits), "%s: bit counts changed inside the timed region" % tag
            assert torch.equal(d_out, ref_out), "%s: output bytes changed inside the timed region" % tag
        return bits, checked

    # isolated call: the parity gate before the timed region, and the copy the region is compared with
    step(0)
    sync()
    other_gate = gate_other_quality(enc, torch, dev) if rank == 0 else None
    ref_bits, n_gold = verify_outputs("before the timed region")
    ref_out = d_out.clone()
    d_out.zero_()
    d_bits.zero_()

    for i in range(args.warmup):
        step(i)
    sync()

    # HIP events around the block-encode kernel launches of every call of the timed region, recorded by
    # the library on the launch stream (mode 2: two records per call)
    enc.set_profiling(2)
    # markers for tools/profile_summary.py: a 256-byte k_lcg_fill launch on either side of the timed region (outside it: the
    # region starts and ends on a device sync), so that a kernel trace of this command says WHICH launches were timed --
    # the parts of a batch differ in size since round 4, so durations alone no longer do
    marker = torch.empty(256, dtype=torch.uint8, device=dev)
    enc.synth_lcg_device(marker.data_ptr(), 256, 1, 0x7ffffff1)
    dt = timed_region(step, args.steps, dist, distributed, sync)
    enc.synth_lcg_device(marker.data_ptr(), 256, 1, 0x7ffffff2)
    enc.sync()
    prof, calls = enc.profile_summary()
    enc.set_profiling(0)
    dt, per_rank = gather_times(dt, dist, distributed, coll_dev)
    _, n_gold_after = verify_outputs("after the timed region", ref_bits, ref_out)
    del ref_out
    if args.dump_outputs:  # before the secondary legs below reuse d_out
        dump_outputs(args.dump_outputs, d_out, ref_bits, rank, world)
    nb0 = int(ref_bits[0])
    scan0 = d_out[0, :(nb0 + 7) // 8].cpu().numpy()  # frame 0 as the timed region wrote it (the legs below reuse d_out)

    line = None
    if rank == 0:
        parts = enc.last_call_parts() if hasattr(enc, "last_call_parts") else None
        total_px = float(args.gpus) * args.steps * F * W * H
        alg_frame = FBYTES + float(np.mean((ref_bits + 7) // 8))  # RGB read once + stream written once
        launches = max(calls, 1) * (parts or 1)
        frames_per_launch = F / float(parts or 1)
        t_launch = prof["transform_ms"] / launches * 1e-3          # average duration of one k_screen_encode launch
        alg_launch = alg_frame * frames_per_launch
        achieved = alg_launch / t_launch / 1e9
        units = (W // 8) * (H // 8) * 3
        # HBM bytes / VALU instructions per FRAME from the PMC passes committed under profiles/
        # (FETCH_SIZE / WRITE_SIZE in separate passes, corrected as MI355X_MICROARCH.md prescribes).
        # They describe the kernel sources they were measured on: null when those have changed.
        traffic = valu = None
        traffic_src = None
        try:
            tj = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
            if tj.get("kernel_sources_sha") == kernel_sources_sha():
                traffic = tj.get("k_screen_encode_hbm_bytes_per_frame")
                valu = tj.get("k_screen_encode_valu_insts_per_frame")
                traffic_src = tj.get("source")
            else:
                traffic_src = "stale: profiles/traffic.json was measured on other kernel sources (%s)" % tj.get("kernel_sources_sha")
        except Exception:
            pass
        line = {
            "metric": "Mpixels/s encode (3840x2160 RGB, q=50)",
            "value": round(total_px / dt / 1e6, 2), "unit": "Mpixel/s",
            "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 5),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": DTYPE, "data": "synthetic",
            "config": {"workload": "configs[1] batched: %d distinct 3840x2160 synthetic RGB frames per step in ONE call "
                                   "(LCG noise, seeds %d.. per rank), q=50 tables, chroma averaging on, strict "
                                   "(bit-exact) mode, device-resident RGB -> packed scan bits, one HIP stream" % (F, 1),
                       "frames_per_step": F, "ms_per_frame": round(dt / args.steps / F * 1e3, 5),
                       "launches_of_dominant_kernel_per_step": parts,
                       "sharding": "frames across ranks, no collective",
                       "launcher": "bench.py (own worker processes)" if os.environ.get("MI355_BENCH_SPAWNED") else
                                   ("external (torchrun)" if distributed else "single process")},
            "ranks_seen": dist.get_world_size() if distributed else 1,
            "collective_backend": (args.backend + (" (RCCL)" if args.backend == "nccl" else "")) if distributed else None,
            "per_rank_mpixel_s": [round(args.steps * F * W * H / t / 1e6, 1) for t in per_rank],
            "verified": {"frames_vs_reference_sha_before": n_gold, "frames_vs_reference_sha_after": n_gold_after,
                         "all_frames_bytes_equal_isolated_call_after_region": True,
                         "second_operating_point_before": other_gate},
            "roofline": {"bound": "valu_issue",
                         "limited_by": "instruction issue of the two resident waves per SIMD (see `binding` and `valu_issue`); achieved / peak / frac "
                                       "below are SURVEY §8(d)'s algorithmic bytes against the HBM roof -- what the metric is priced "
                                       "against, not what binds the kernel",
                         "achieved": round(achieved, 2), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBPS, 5), "hbm_frac": round(achieved / HBM_PEAK_GBPS, 5),
                         "traffic": None if traffic is None else int(traffic * frames_per_launch),
                         "traffic_source": traffic_src,
                         "kernel": "k_screen_encode", "kernel_ms": round(t_launch * 1e3, 5),
                         "frames_per_launch": frames_per_launch,
                         "kernel_ms_per_frame": round(t_launch * 1e3 / frames_per_launch, 5),
                         "algorithmic_bytes_per_launch": int(alg_launch),
                         "launches_timed": launches,
                         "kernel_ms_scope": "HIP events on the launch stream inside the timed region, one bracket per "
                                            "call spanning its back-to-back k_screen_encode launches (nothing else is "
                                            "on that stream between them), divided by the launches; the tail kernels of "
                                            "earlier parts run concurrently on the library's side stream",
                         "binding": "VALU instruction issue, not HBM and not the matrix pipe: bit-exact strict mode "
                                    "evaluates the reference's order-dependent fp64 chain as an exact integer-MFMA map "
                                    "+ verification, and the per-unit entropy walk is instruction bound (DESIGN.md §4.4)",
                         "whole_pipeline": {"achieved": round(alg_frame * F / (dt / args.steps) / 1e9, 2), "unit": "GB/s",
                                            "frac": round(alg_frame * F / (dt / args.steps) / 1e9 / HBM_PEAK_GBPS, 5),
                                            "note": "algorithmic bytes of a step / ms_per_step (all kernels, wall clock)"}},
            "equivalent_reference_fp64": {"value": round(units * frames_per_launch * ALG_FP64_OPS_PER_UNIT / t_launch / 1e12, 3),
                                          "unit": "Top/s",
                                          "note": "unfused fp64 mul/add the reference's in-place chain would need for the "
                                                  "same frames (units*12416 per frame) per second of this kernel; the "
                                                  "vector-FP64 peak is 39.3 Top/s unfused -- the kernel does not execute "
                                                  "these ops, it replaces them"},
        }
        if valu:
            # informational: what actually binds the kernel.  A CDNA4 SIMD is 32 lanes wide, a wave64 VALU
            # instruction holds it for 2 cycles: peak = 256 CUs x 4 SIMDs x 2.4 GHz / 2 wave-instructions/s.
            peak = 256 * 4 * 2.4e9 / 2 / 1e12
            rate = valu * frames_per_launch / t_launch / 1e12
            # The same rate priced at what the kernel's instruction mix costs at its two waves per SIMD on this chip
            # (tools/microbench/valu_issue.hip, profiles/r03_e_valu_issue_microbench.txt: 2.9 SIMD cycles for plain
            # add/logic/shift, 3.6 with an SGPR source / conversions, 3.9 for integer multiply, permute and three-operand
            # forms; ~3.6 for this mix) instead of the 2 cycles of the SIMD-32 model.
            mix_cycles = 3.6
            line["valu_issue"] = {"achieved": round(rate, 4), "peak": round(peak, 4), "unit": "T wave-instructions/s",
                                  "frac": round(rate / peak, 4), "insts_per_frame": valu, "source": traffic_src,
                                  "measured_cost_model": {"simd_cycles_per_instruction": mix_cycles, "waves_per_simd": 2,
                                                          "peak": round(peak * 2 / mix_cycles, 4),
                                                          "frac": round(rate / (peak * 2 / mix_cycles), 4),
                                                          "source": "profiles/r03_e_valu_issue_microbench.txt"}}

    # ---- secondary measurements (rank 0, after the region; none of them is `value`) ---------------------
    if rank == 0 and not args.quick:
        if args.gpus == 1:
            line["single_call_latency_ms"] = single_call_latency(enc, d_rgb, d_out, d_bits, cap, stream, torch)
            try:
                line["standard_mode"] = standard_mode_leg(jpeg, enc, d_rgb, d_out, d_bits, cap, stream, F, torch, args)
            except Exception as exc:  # pragma: no cover
                line["standard_mode"] = {"error": str(exc)}
        try:
            line["other_configs"] = other_configs_leg(jpeg, enc, torch, dev, stream)
        except Exception as exc:  # pragma: no cover
            line["other_configs"] = {"error": repr(exc)}
        try:  # all the run's GPUs through the pool (the other ranks are idle on the CPU by now)
            devs = [r if not args.share_device else r % max(ndev, 1) for r in range(args.gpus)]
            line["end_to_end"] = end_to_end_leg(jpeg, d_rgb, devs, torch, golden, seed0)
        except Exception as exc:  # pragma: no cover
            line["end_to_end"] = {"error": str(exc)}
    if rank == 0 and not args.no_cpu_baseline:
        base, r = cpu_baseline()
        # the CPU path's bits for seed 1 against what the GPU wrote in the timed region
        assert r.n_bits == nb0 and np.array_equal(np.asarray(r.bits), scan0), \
            "GPU scan of frame seed 1 differs from the CPU path run in this process"
        line["cpu_baseline"] = base
        try:  # extra, never the reported baseline: all host threads at once
            line["cpu_baseline_all_threads"] = cpu_baseline_multicore()
        except Exception as exc:  # pragma: no cover
            line["cpu_baseline_all_threads"] = {"error": str(exc)}
    if rank == 0:
        print(json.dumps(line), flush=True)

    enc.close()
    if distributed:
        dist.barrier(group=tail_group) if tail_group is not None else dist.barrier()
        dist.destroy_process_group()


def single_call_latency(enc, d_rgb, d_out, d_bits, cap, stream, torch):
    """One 4K frame per call, one call at a time on the whole device: median wall time of call + sync."""
    ts = []
    for i in range(30):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enc.encode_scan_device(d_rgb.data_ptr(), W, H, 1, d_out.data_ptr(), cap, d_bits.data_ptr(), stream=stream)
        enc.sync(stream)
        ts.append(time.perf_counter() - t0)
    return round(float(np.median(ts[5:])) * 1e3, 5)


def standard_mode_leg(jpeg, enc, d_rgb, d_out, d_bits, cap, stream, F, torch, args):
    """The decodable baseline mode (NOT a behaviour of the reference): real 4:2:0 MCUs, true
    DCT-II, Annex K tables; same batch, same call shape."""
    flags = jpeg.F_STANDARD | jpeg.F_420
    steps = max(2, min(args.steps, 10))

    def go():
        enc.encode_scan_device(d_rgb.data_ptr(), W, H, F, d_out.data_ptr(), cap, d_bits.data_ptr(), flags=flags, stream=stream)

    go()
    enc.sync(stream)
    enc.set_profiling(2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        go()
    enc.sync(stream)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    prof, calls = enc.profile_summary()
    enc.set_profiling(0)
    bits = d_bits.cpu().numpy().astype(np.int64)
    alg = FBYTES + float(np.mean((bits + 7) // 8))
    gbps = alg * F / dt / 1e9
    t_k = prof["transform_ms"] / max(calls, 1) * 1e-3
    return {"value": round(F * W * H / dt / 1e6, 2), "unit": "Mpixel/s", "flags": "MI355_F_STANDARD|MI355_F_420",
            "frames_per_call": F, "ms_per_call": round(dt * 1e3, 4), "bits_per_pixel": round(float(bits.mean()) / (W * H), 4),
            "algorithmic_bytes_per_frame": int(alg), "achieved_GBps": round(gbps, 1), "frac_of_hbm_peak": round(gbps / HBM_PEAK_GBPS, 5),
            "block_encode_kernel_ms_per_call": round(t_k * 1e3, 4),
            "block_encode_kernel_GBps": round(alg * F / t_k / 1e9, 1),
            "note": "parity of this mode is pinned by the checker + Pillow decode in tests/test_standard_mode.py, not by the "
                    "reference (which has no decodable mode); bound by VALU issue in colour conversion + quantiser + "
                    "entropy walk like the strict kernel (DESIGN.md §4.6)"}


def end_to_end_leg(jpeg, d_rgb, device_ids, torch, golden, seed0, per_gpu=48):
    """PCIe-inclusive secondary figure: frames in pinned host memory -> scans in pinned host memory through
    mi355_jpeg_pool_encode over `device_ids` (one worker per GPU: chunked H2D || encode || D2H on three streams each;
    frames sharded over the workers, no collective)."""
    import ctypes as C
    ndev = len(device_ids)
    src = min(per_gpu, d_rgb.shape[0])
    n = src * ndev
    h_rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, pin_memory=True)
    for k in range(ndev):  # every GPU's share is a copy of rank 0's first frames
        h_rgb[k * src:(k + 1) * src].copy_(d_rgb[:src])
    cap = 6 << 20
    h_out = torch.empty((n, cap), dtype=torch.uint8, pin_memory=True)
    bits = (C.c_uint64 * n)()
    secs = C.c_double()
    pool = jpeg.Pool(list(device_ids))
    pool.set_quality(QUALITY)
    best = None
    for _ in range(3):
        rc = jpeg.lib().mi355_jpeg_pool_encode(pool._h, h_rgb.data_ptr(), W, H, n, jpeg.F_DEFAULT, h_out.data_ptr(), cap,
                                               bits, C.byref(secs))
        assert rc == 0, rc
        best = secs.value if best is None else min(best, secs.value)
    counts = pool.debug_counts()
    pool.close()
    g = golden.get(seed0)
    if g is not None:
        for k in range(ndev):
            nb = int(bits[k * src])
            assert nb == g[0] and ascii_sha(h_out[k * src, :(nb + 7) // 8].numpy(), nb) == g[1], "end-to-end scan differs from the reference"
    out_bytes = sum((int(b) + 7) // 8 for b in bits)
    return {"value": round(n * W * H / best / 1e6, 1), "unit": "Mpixel/s", "frames": n, "gpus": ndev,
            "per_gpu_mpixel_s": round(n * W * H / best / 1e6 / ndev, 1),
            "h2d_GBps_per_gpu": round(n * FBYTES / best / 1e9 / ndev, 2), "d2h_GBps_per_gpu": round(out_bytes / best / 1e9 / ndev, 2),
            "seconds": round(best, 5),
            "pool_objects_created": {"allocations": counts[0], "host_registrations": counts[1], "streams_events": counts[2], "calls": counts[3]},
            "note": "PCIe-inclusive: pinned host RGB in, host scan bytes out, every GPU of the run through one persistent pool, "
                    "best of 3 calls; the link is the limit here, not the kernels -- secondary figure, never `value`"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames-per-step", type=int, default=128,
                    help="distinct resident 4K frames encoded by the one call of a step")
    ap.add_argument("--cap-mb", type=int, default=8, help="output capacity per frame slot in MiB")
    ap.add_argument("--verify-frames", type=int, default=4, help="frames per rank re-hashed against the reference goldens")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--quick", action="store_true", help="skip the secondary legs (latency, standard mode, end to end)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last one computed (per-frame scan bit counts and a fixed "
                         "seeded sample of the scan bytes) as DIR/<name>.npy in float64/float32, at most 64 MB in all")
    ap.add_argument("--worker-timeout", type=float, default=1500.0)
    ap.add_argument("--dead-rank-grace", type=float, default=30.0, help=argparse.SUPPRESS)
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl", help=argparse.SUPPRESS)
    ap.add_argument("--share-device", action="store_true", help=argparse.SUPPRESS)  # rehearsal: ranks share the box's GPU(s)
    ap.add_argument("--dry-run-cpu", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--rehearse-dist", action="store_true", help=argparse.SUPPRESS)  # N = 1 through the process-group code path
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(launch_workers(args, sys.argv[1:]))
    if args.dry_run_cpu:
        return dry_run_cpu(args)
    return worker(args)


if __name__ == "__main__":
    main()
