"""Grayscale (one-component) baseline JPEG in standard mode: MI355_F_GRAY.

The checker is the one standard mode already has.  The luma row of its colour conversion sums to 2^15, so the luma of
(g,g,g) is g exactly, and the coefficients of a gray frame are bit for bit the luma rows (the first N rows of the
reference row order) of oracle_std_encode run on (g,g,g).  The expected scan is built here from those rows with the
Annex K luma tables (K.3, K.5): DC differences, ZRL, EOB omitted after a non-zero coefficient 63.  The CPU tests pin
that builder against an independent decoder (PIL) before the GPU tests compare the library with it."""
import importlib
import io
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from conftest import GOLD, ROOT

PIL = pytest.importorskip("PIL.Image")
jpeg_mod = importlib.import_module("jpeg-encoder-opencl_amd")
F_STD, F_GRAY, F_420, F_RESTART = 2, 16, 4, 8
GRAY = F_STD | F_GRAY

# the builder (Annex K luma tables, entropy coder, one-component container, checker rows) lives in oracle_lib
entropy_code, jfif_gray, checker_rows = ol.gray_entropy_code, ol.jfif_gray, ol.gray_checker_rows


def expected(gray, quality):
    ql, qc = ol.quant_tables(quality)
    rows = checker_rows(gray, ql, qc)
    packed, n_bits = entropy_code(rows)
    return rows, packed, n_bits


# ---------------------------------------------------------------- inputs
def smooth_gray(W, H, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    img = 127 + 90 * np.sin(x / 37.0 + seed) * np.cos(y / 23.0) + 30 * np.cos(x / 11.0 + y / 29.0)
    img += rng.normal(0, 2, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def lcg_gray(W, H, seed=1):
    buf = np.empty(W * H, np.uint8)
    ol.oracle().orc_lcg_fill(buf.ctypes.data, buf.size, seed)
    return buf.reshape(H, W)


def fruit_luma():
    rgb = ol.read_ppm(os.path.join(GOLD, "fruit.ppm"))
    return ol.std_csc(rgb)[..., 0].astype(np.uint8)


def extremes_gray(W, H, seed=7):
    return np.random.default_rng(seed).choice(np.array([0, 1, 254, 255], np.uint8), size=(H, W))


CASES = {  # name: (frame builder, quality)
    "fruit_luma_q50": (fruit_luma, 50),
    "lcg_640x360_q50": (lambda: lcg_gray(640, 360), 50),
    "smooth_100x37_q90": (lambda: smooth_gray(100, 37, 1), 90),
    "smooth_1920x1080_q75": (lambda: smooth_gray(1920, 1080, 2), 75),
    "lcg_8x8_q100": (lambda: lcg_gray(8, 8, 3), 100),
    "smooth_333x65_q25": (lambda: smooth_gray(333, 65, 4), 25),
    "smooth_3840x2160_q50": (lambda: smooth_gray(3840, 2160, 5), 50),
    "lcg_65535x9_q50": (lambda: lcg_gray(65535, 9, 6), 50),
    "extremes_2048x72_q50": (lambda: extremes_gray(2048, 72), 50),
}


def psnr(a, b):
    mse = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()
    return 10 * np.log10(255.0 ** 2 / mse)


def decode_l(data):
    im = PIL.open(io.BytesIO(data))
    assert im.mode == "L", im.mode
    return np.asarray(im)


# ---------------------------------------------------------------- CPU: the builder, the bound, the flag mask
@pytest.mark.parametrize("W,H,quality", [(253, 254, 90), (333, 65, 90), (640, 360, 75)])
def test_builder_files_decode_as_gray_and_match_an_independent_encoder(W, H, quality):
    gray = smooth_gray(W, H, W)
    ql, _ = ol.quant_tables(quality)
    _, packed, n_bits = expected(gray, quality)
    ours = decode_l(jfif_gray(packed, n_bits, W, H, ql))
    assert ours.shape == (H, W)
    assert psnr(ours, gray) > 35.0
    buf = io.BytesIO()
    PIL.fromarray(gray, "L").save(buf, "JPEG", qtables=[[int(v) for v in ql.reshape(64)]])
    theirs = decode_l(buf.getvalue())
    assert psnr(ours, theirs) > 45.0


def test_builder_agrees_with_the_checker_on_the_luma_of_an_rgb_scan():
    """On (g,g,g) the 4:4:4 scan of the checker interleaves these luma units with all-zero chroma units; the luma
    rows alone, coded by the builder, are what the first components' symbols say (a check of the builder's code
    tables against the checker's own: the 4:4:4 scan must contain exactly builder bits + 2 x N chroma units of
    DC 0 / EOB (2 + 2 bits each))."""
    gray = smooth_gray(64, 40, 3)
    ql, qc = ol.quant_tables(50)
    o = ol.oracle_std_encode(np.repeat(gray[:, :, None], 3, 2), ql, qc, keep=ol.KEEP_ZIGZAG)
    N = 8 * 5
    assert not o.zigzag[N:].any()  # chroma of a gray picture is flat
    _, n_bits = entropy_code(o.zigzag[:N])
    assert o.n_bits == n_bits + 2 * N * (2 + 2)


def test_scan_bound_flags_gray(jpeg):
    for W, H in [(8, 8), (253, 254), (3840, 2160), (65535, 9)]:
        blocks = ((W + 7) // 8) * ((H + 7) // 8)
        g = jpeg.scan_bound(W, H, GRAY)
        assert g * 8 >= blocks * 1727
        assert g < jpeg.scan_bound(W, H, F_STD)
        gr = jpeg.scan_bound(W, H, GRAY | F_RESTART)
        assert gr * 8 >= blocks * 1727 + ((blocks + 63) // 64) * 7
        assert gr < jpeg.scan_bound(W, H, F_STD | F_RESTART)


def test_supported_flags(jpeg):
    assert jpeg.F_GRAY == 16
    assert jpeg.supported_flags() == 0x1F


def _write_pgm(path, gray, comment=True):
    H, W = gray.shape
    with open(path, "wb") as f:
        f.write(b"P5\n" + (b"# gray test frame\n" if comment else b"") + b"%d %d\n255\n" % (W, H) + gray.tobytes())


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def genc():
    e = jpeg_mod.Encoder(0)  # a context of its own: these tests change the quality
    yield e
    e.close()


_EXPECTED = {}


def _case(name):
    if name not in _EXPECTED:
        make, quality = CASES[name]
        gray = np.ascontiguousarray(make())
        _EXPECTED[name] = (gray, quality) + expected(gray, quality)
    return _EXPECTED[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_coefficients_equal_the_checker_luma_rows(genc, name):
    gray, quality, rows, _, _ = _case(name)
    genc.set_quality(quality)
    got = genc.probe_coefficients(gray, GRAY)
    assert got.shape == rows.shape
    assert np.array_equal(got, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_scan_equals_the_builder(genc, name):
    gray, quality, _, packed, n_bits = _case(name)
    genc.set_quality(quality)
    bits, nb = genc.encode_scan(gray, GRAY)
    assert nb[0] == n_bits
    assert np.array_equal(bits[0], packed[:(n_bits + 7) // 8])


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(8, 8), (253, 254), (333, 65), (640, 360), (17, 9)])
def test_samples_are_the_mirror_padded_input(genc, W, H):
    gray = lcg_gray(W, H, W + H)
    got = genc.probe_samples(gray, GRAY)
    W8, H8 = (W + 7) // 8 * 8, (H + 7) // 8 * 8
    assert got.shape == (H8, W8)
    assert np.array_equal(got, np.pad(gray, ((0, H8 - H), (0, W8 - W)), mode="symmetric"))


def _device_batch(enc, frames, cap, flags=GRAY):
    import torch
    n, H, W = frames.shape
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    d_out = torch.zeros((n, cap), dtype=torch.uint8, device=dev)
    d_bits = torch.zeros(n, dtype=torch.int64, device=dev)
    enc.encode_scan_device(d_in.data_ptr(), W, H, n, d_out.data_ptr(), cap, d_bits.data_ptr(), flags)
    err = None
    try:
        enc.sync()
    except jpeg_mod.JpegError as e:
        err = e.status
    return d_bits.cpu().numpy().astype(np.uint64), d_out.cpu().numpy(), err


@pytest.mark.gpu
def test_batch_of_distinct_frames_equals_single_frames(genc):
    genc.set_quality(75)
    W, H, n = 333, 65, 37
    frames = np.stack([smooth_gray(W, H, 100 + f) if f % 2 else lcg_gray(W, H, 100 + f) for f in range(n)])
    cap = (jpeg_mod.scan_bound(W, H, GRAY) + 3) & ~3
    bits, out, err = _device_batch(genc, frames, cap)
    assert err is None
    for f in range(n):
        one, nb = genc.encode_scan(frames[f], GRAY)
        assert int(bits[f]) == nb[0], f
        assert np.array_equal(out[f, :(nb[0] + 7) // 8], one[0]), f


@pytest.mark.gpu
def test_large_batch_across_parts_equals_single_frames(genc):
    """64 4K gray frames: several parts (cut by pixels) and the workspace sets they use."""
    genc.set_quality(50)
    W, H, n = 3840, 2160, 64
    frames = np.stack([smooth_gray(W, H, f) if f % 3 else lcg_gray(W, H, f) for f in range(n)])
    cap = (W * H // 2 + 4096 + 3) & ~3
    bits, out, err = _device_batch(genc, frames, cap)
    assert err is None
    assert genc.last_call_parts() > 1
    for f in range(0, n, 1):
        one, nb = genc.encode_scan(frames[f], GRAY)
        assert int(bits[f]) == nb[0], f
        assert np.array_equal(out[f, :(nb[0] + 7) // 8], one[0]), f


@pytest.mark.gpu
def test_frames_over_capacity_are_flagged_and_the_others_intact(genc):
    genc.set_quality(100)
    W, H, n = 256, 64, 12
    frames = np.stack([smooth_gray(W, H, f) for f in range(n)])
    offenders = (2, 3, 9)
    for f in offenders:
        frames[f] = lcg_gray(W, H, 300 + f)  # q100 noise: far more bits than the smooth frames
    single = {f: genc.encode_scan(frames[f], GRAY) for f in range(n) if f not in offenders}
    cap = ((max(nb[0] for _, nb in single.values()) + 7) // 8 + 64 + 3) & ~3
    bits, out, err = _device_batch(genc, frames, cap)
    assert err == jpeg_mod.E_CAPACITY
    for f in range(n):
        if f in offenders:
            assert bits[f] == np.uint64(jpeg_mod.BITS_CAPACITY), f
        else:
            one, nb = single[f]
            assert int(bits[f]) == nb[0] and np.array_equal(out[f, :(nb[0] + 7) // 8], one[0]), f


def _segments(data):
    """[(marker, payload)] of the header, then the entropy-coded bytes."""
    pos, segs = 2, []
    while True:
        m = data[pos + 1]
        length = int.from_bytes(data[pos + 2:pos + 4], "big")
        segs.append((m, data[pos + 4:pos + 2 + length]))
        pos += 2 + length
        if m == 0xDA:
            return segs, data[pos:-2]


@pytest.mark.gpu
def test_files(genc):
    genc.set_quality(75)
    gray = smooth_gray(333, 200, 9)
    H, W = gray.shape
    f = genc.encode_jfif(gray, GRAY)
    bits, nb = genc.encode_scan(gray, GRAY)
    assert f == genc.wrap_jfif(bits[0], nb[0], W, H, GRAY)
    segs, _ = _segments(f)
    markers = [m for m, _ in segs]
    assert markers.count(0xDB) == 1 and markers.count(0xC4) == 2 and 0xDD not in markers
    sof = dict(segs)[0xC0]
    assert sof[5] == 1 and bytes(sof[6:9]) == b"\x01\x11\x00"
    pixels = decode_l(f)
    assert pixels.shape == (H, W) and psnr(pixels, gray) > 35.0
    # with restart intervals: DRI 64, RST0..7 cycling between the tiles, the same picture
    fr = genc.encode_jfif(gray, GRAY | F_RESTART)
    segs, ecs = _segments(fr)
    assert dict(segs)[0xDD] == b"\x00\x40"
    tiles = (((W + 7) // 8) * ((H + 7) // 8) + 63) // 64
    rst = [ecs[i + 1] for i in range(len(ecs) - 1) if ecs[i] == 0xFF and ecs[i + 1] != 0x00]
    assert rst == [0xD0 + (k & 7) for k in range(tiles - 1)]
    assert np.array_equal(decode_l(fr), pixels)


@pytest.mark.gpu
def test_refusals(genc, jpeg):
    gray = smooth_gray(64, 64)
    for flags in (F_GRAY, F_GRAY | 1, GRAY | F_420):
        with pytest.raises(jpeg.JpegError) as ei:
            genc.encode_scan(gray, flags)
        assert ei.value.status == jpeg.E_ARG, flags
    with pytest.raises(jpeg.JpegError) as ei:
        genc.probe_unit_bits(gray, GRAY)
    assert ei.value.status == jpeg.E_ARG
    with pytest.raises(jpeg.JpegError) as ei:
        genc.probe_unit_bits(gray, F_GRAY)
    assert ei.value.status == jpeg.E_ARG


@pytest.mark.gpu
def test_pool_equals_the_encoder(genc):
    genc.set_quality(50)
    W, H, n = 640, 360, 10
    frames = np.stack([lcg_gray(W, H, 40 + f) if f % 2 else smooth_gray(W, H, 40 + f) for f in range(n)])
    pool = jpeg_mod.Pool([0, 0])
    try:
        out, bits, _ = pool.encode(frames, GRAY)
    finally:
        pool.close()
    for f in range(n):
        one, nb = genc.encode_scan(frames[f], GRAY)
        assert bits[f] == nb[0], f
        assert np.array_equal(out[f, :(nb[0] + 7) // 8], one[0]), f


@pytest.mark.gpu
def test_interleaved_modes_on_one_context():
    """strict -> gray -> RGB standard 4:2:0 -> gray on one context: each result equals a fresh context's."""
    rgb = ol.lcg_frame(640, 360, 3)
    g1, g2 = smooth_gray(1920, 1080, 1), lcg_gray(333, 65, 2)
    calls = [(rgb, 1), (g1, GRAY), (rgb, F_STD | F_420), (g2, GRAY | F_RESTART)]
    shared = jpeg_mod.Encoder(0)
    try:
        got = [shared.encode_scan(x, fl) for x, fl in calls]
    finally:
        shared.close()
    for (x, fl), (bits, nb) in zip(calls, got):
        fresh = jpeg_mod.Encoder(0)
        try:
            fb, fn = fresh.encode_scan(x, fl)
        finally:
            fresh.close()
        assert nb == fn and np.array_equal(bits[0], fb[0]), fl


@pytest.mark.gpu
def test_cli_encodes_pgm(tmp_path):
    cli = os.path.join(ROOT, "jpeg-encoder-opencl_amd", "host", "mi355-jpeg")
    gray = smooth_gray(333, 65, 11)
    pgm = tmp_path / "scan.pgm"
    _write_pgm(pgm, gray)
    out = tmp_path / "scan.jpg"
    r = subprocess.run([cli, str(pgm), str(out), "--mode", "standard", "-q", "85"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    ql, _ = ol.quant_tables(85)
    _, packed, n_bits = expected(gray, 85)
    assert np.array_equal(decode_l(out.read_bytes()), decode_l(jfif_gray(packed, n_bits, 333, 65, ql)))
    r = subprocess.run([cli, str(pgm), str(tmp_path / "strict.jpg"), "--mode", "strict"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0
    assert "standard" in r.stdout
    assert not (tmp_path / "strict.jpg").exists()
