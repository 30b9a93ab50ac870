"""ctypes bindings for the test oracle (oracle/liboracle.so) and, where it has been
built (this container only), the real reference library (oracle/_ref/libjpegref.so).

TEST INFRASTRUCTURE: imported by tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg only.  The product package never imports this module.
"""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")

KEEP_ZIGZAG, KEEP_UNIT_BITS, KEEP_U8_STAGES, KEEP_DCT = 1, 2, 4, 8


class OrcResult(C.Structure):
    _fields_ = [
        ("W8", C.c_size_t), ("H8", C.c_size_t), ("n_blocks", C.c_size_t),
        ("n_bits", C.c_uint64), ("bits", C.POINTER(C.c_uint8)), ("bits_bytes", C.c_size_t),
        ("zigzag", C.POINTER(C.c_int32)), ("unit_bits", C.POINTER(C.c_uint32)),
        ("csc", C.POINTER(C.c_uint8)), ("cds", C.POINTER(C.c_uint8)),
        ("padded", C.POINTER(C.c_uint8)), ("dct", C.POINTER(C.c_double)),
        ("stage_us", C.c_double * 9),
    ]


_oracle = None
_ref = None


def build_oracle():
    subprocess.check_call(["make", "-s", "-C", ORACLE_DIR, "all"])


def oracle():
    global _oracle
    if _oracle is None:
        path = os.path.join(ORACLE_DIR, "liboracle.so")
        if not os.path.exists(path):
            build_oracle()
        L = C.CDLL(path)
        L.orc_cos.restype = C.c_double
        L.orc_cos.argtypes = [C.c_int, C.c_int]
        L.orc_scale.restype = C.c_double
        L.orc_scale.argtypes = [C.c_int, C.c_int]
        L.orc_encode.restype = C.c_int
        L.orc_encode.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                 C.c_int, C.c_int, C.POINTER(OrcResult)]
        L.orc_result_free.argtypes = [C.POINTER(OrcResult)]
        L.orc_huff_code.restype = C.c_int
        L.orc_huff_code.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32)]
        L.orc_entropy.restype = C.c_int
        L.orc_entropy.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.POINTER(C.c_uint8)),
                                  C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), C.c_void_p]
        L.orc_lcg_fill.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32]
        L.orc_std_encode.restype = C.c_int
        L.orc_std_encode.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int, C.c_int, C.POINTER(OrcResult)]
        L.orc_std_csc.restype = None
        L.orc_std_csc.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        L.orc_std_jfif_restart.restype = C.c_long
        L.orc_std_jfif_restart.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_int, C.c_uint, C.c_void_p, C.c_size_t]
        L.orc_jfif_frame_s.restype = C.c_long
        L.orc_jfif_frame_s.argtypes = [C.c_void_p, C.c_uint64, C.c_size_t, C.c_size_t, C.c_void_p,
                                       C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.orc_jfif_frame.restype = C.c_long
        L.orc_jfif_frame.argtypes = [C.c_void_p, C.c_uint64, C.c_size_t, C.c_size_t, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_size_t]
        L.orc_dct_block.argtypes = [C.c_void_p]
        L.orc_dct_blocks.argtypes = [C.c_void_p, C.c_size_t]
        L.orc_quant_block.argtypes = [C.c_void_p, C.c_void_p]
        L.orc_csc.argtypes = [C.c_void_p, C.c_size_t]
        L.orc_cds.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t]
        L.orc_zigzag_order.argtypes = [C.c_void_p]
        L.orc_quant_q50.argtypes = [C.c_void_p, C.c_void_p]
        L.orc_quant_ijg.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        _oracle = L
    return _oracle


def ref_available():
    return os.path.exists(os.path.join(ORACLE_DIR, "_ref", "libjpegref.so"))


def ref():
    """The real reference stage library (built in this container from
    the reference's own utils.cpp in place).  None when not built/loadable."""
    global _ref
    if _ref is None:
        path = os.path.join(ORACLE_DIR, "_ref", "libjpegref.so")
        if not os.path.exists(path):
            return None
        try:
            L = C.CDLL(path)
        except OSError:
            return None
        L.ref_run.restype = C.c_void_p
        L.ref_run.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                              C.c_int, C.c_int]
        L.ref_free.argtypes = [C.c_void_p]
        L.ref_dims.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        for name, rt in [("ref_csc", C.POINTER(C.c_uint8)), ("ref_cds", C.POINTER(C.c_uint8)),
                         ("ref_padded", C.POINTER(C.c_uint8)), ("ref_dct", C.POINTER(C.c_double)),
                         ("ref_zigzag", C.POINTER(C.c_int32)), ("ref_nbits", C.c_uint64),
                         ("ref_bits", C.POINTER(C.c_char)),
                         ("ref_stage_us", C.POINTER(C.c_double))]:
            f = getattr(L, name)
            f.restype = rt
            f.argtypes = [C.c_void_p]
        L.ref_csc_only.argtypes = [C.c_void_p, C.c_size_t]
        L.ref_quant_tables.argtypes = [C.c_void_p, C.c_void_p]
        L.ref_huff_code.restype = C.c_int
        L.ref_huff_code.argtypes = [C.c_int, C.c_int, C.c_int, C.c_char_p]
        L.ref_cos.restype = C.c_double
        L.ref_cos.argtypes = [C.c_size_t, C.c_size_t]
        L.ref_scale.restype = C.c_double
        L.ref_scale.argtypes = [C.c_size_t, C.c_size_t]
        _ref = L
    return _ref


# ---------------------------------------------------------------- helpers

def quant_tables(quality=50):
    """(qlum, qchrom) uint32[64] row-major [v][u].  quality 50 = the reference's
    tables (utils.hpp:42-62); anything else = IJG scaling (build convention)."""
    ql = np.zeros(64, np.uint32)
    qc = np.zeros(64, np.uint32)
    if quality == 50:
        oracle().orc_quant_q50(ql.ctypes.data, qc.ctypes.data)
    else:
        oracle().orc_quant_ijg(quality, ql.ctypes.data, qc.ctypes.data)
    return ql, qc


def lcg_frame(W, H, seed=1):
    """Pinned synthetic frame of SURVEY §8d: uint8 [H, W, 3]."""
    buf = np.empty(W * H * 3, np.uint8)
    oracle().orc_lcg_fill(buf.ctypes.data, buf.size, seed)
    return buf.reshape(H, W, 3)


def read_ppm(path):
    """Minimal P6 reader for the reference's 3-line header form (utils.cpp:11-65)."""
    with open(path, "rb") as f:
        data = f.read()
    assert data[:3] == b"P6\n"
    pos = 3
    while data[pos:pos + 1] == b"#":
        pos = data.index(b"\n", pos) + 1
    end = data.index(b"\n", pos)
    W, H = (int(t) for t in data[pos:end].split())
    pos = end + 1
    end = data.index(b"\n", pos)
    assert int(data[pos:end]) == 255
    pos = end + 1
    return np.frombuffer(data, np.uint8, W * H * 3, pos).reshape(H, W, 3).copy()


class Encoded:
    """Result of one CPU encode, as numpy arrays."""
    pass


def oracle_encode(rgb, qlum=None, qchrom=None, cds_on=True, keep=0):
    rgb = np.ascontiguousarray(rgb, np.uint8)
    H, W, _ = rgb.shape
    if qlum is None:
        qlum, qchrom = quant_tables(50)
    qlum = np.ascontiguousarray(qlum, np.uint32)
    qchrom = np.ascontiguousarray(qchrom, np.uint32)
    res = OrcResult()
    rc = oracle().orc_encode(rgb.ctypes.data, W, H, qlum.ctypes.data, qchrom.ctypes.data,
                             int(cds_on), keep, C.byref(res))
    if rc != 0:
        raise RuntimeError("orc_encode failed: %d" % rc)
    out = Encoded()
    out.W8, out.H8, out.n_blocks, out.n_bits = res.W8, res.H8, res.n_blocks, res.n_bits
    out.bits = np.ctypeslib.as_array(res.bits, (res.bits_bytes,)).copy()
    N = res.n_blocks
    out.zigzag = np.ctypeslib.as_array(res.zigzag, (3 * N, 64)).copy() if res.zigzag else None
    out.unit_bits = np.ctypeslib.as_array(res.unit_bits, (3 * N,)).copy() if res.unit_bits else None
    out.csc = np.ctypeslib.as_array(res.csc, (H, W, 3)).copy() if res.csc else None
    out.cds = np.ctypeslib.as_array(res.cds, (H, W, 3)).copy() if res.cds else None
    out.padded = np.ctypeslib.as_array(res.padded, (res.H8, res.W8, 3)).copy() if res.padded else None
    out.dct = np.ctypeslib.as_array(res.dct, (res.H8, res.W8, 3)).copy() if res.dct else None
    out.stage_us = list(res.stage_us)
    oracle().orc_result_free(C.byref(res))
    return out


def zigzag_order():
    """zz[k] = natural index (v*8+u) of zig-zag position k."""
    zz = np.zeros(64, np.uint8)
    oracle().orc_zigzag_order(zz.ctypes.data)
    return zz


def oracle_entropy(zigzag):
    """performRLE + HuffmanEncoder (the reference's rules) on int32 rows [3N][64]: (packed bits, n_bits)."""
    z = np.ascontiguousarray(zigzag, np.int32)
    N = z.shape[0] // 3
    out, nb, n = C.POINTER(C.c_uint8)(), C.c_size_t(), C.c_uint64()
    rc = oracle().orc_entropy(z.ctypes.data, N, C.byref(out), C.byref(nb), C.byref(n), None)
    if rc != 0:
        raise RuntimeError("orc_entropy failed: %d" % rc)
    return np.ctypeslib.as_array(out, (nb.value,)).copy(), int(n.value)


def std_dct_table():
    """The fixed-point true-DCT table that DEFINES standard mode (tests/golden/std_dct_q39.i64)."""
    return np.fromfile(os.path.join(ROOT, "tests", "golden", "std_dct_q39.i64"), "<i8").reshape(64, 64)


STD_Y = (9798, 19235, 3735)                                     # x 2^-15, sum 2^15
STD_C = ((-5529, -10855, 16384), (16384, -13720, -2664))        # Cb, Cr x 2^-15, each row sums to 0
STD_C420 = ((-2765, -5427, 8192), (8192, -6860, -1332))         # the same / 4 at 16 bits (4:2:0 box filter)


def std_csc(rgb):
    """numpy restatement of standard mode's per-pixel colour conversion (15-bit fixed point, libjpeg's form)."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (STD_Y[0] * r + STD_Y[1] * g + STD_Y[2] * b + 16384) >> 15
    cc = [((c[0] * r + c[1] * g + c[2] * b + 16383) >> 15) + 128 for c in STD_C]
    return np.stack([y] + cc, -1)


def std_chroma420(rgb):
    """4:2:0 chroma of standard mode for an image whose sides are even: the box filter of the linear form over
    each 2x2 quad, rounded once.  Returns (H/2, W/2, 2)."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    out = []
    for c in STD_C420:
        lin = c[0] * r + c[1] * g + c[2] * b
        quad = lin[0::2, 0::2] + lin[0::2, 1::2] + lin[1::2, 0::2] + lin[1::2, 1::2]
        out.append(((quad + 32767) >> 16) + 128)
    return np.stack(out, -1)


def oracle_std_csc(rgb):
    rgb = np.ascontiguousarray(rgb, np.uint8)
    out = np.empty_like(rgb)
    oracle().orc_std_csc(rgb.ctypes.data, rgb.size // 3, out.ctypes.data)
    return out


def oracle_std_encode(rgb, qlum, qchrom, keep=0, subsample=0):
    """Standard (decodable) mode of the test oracle; subsample 0 = 4:4:4, 1 = 4:2:0."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    H, W, _ = rgb.shape
    qlum = np.ascontiguousarray(qlum, np.uint32)
    qchrom = np.ascontiguousarray(qchrom, np.uint32)
    dct = np.ascontiguousarray(std_dct_table(), np.int64)
    res = OrcResult()
    rc = oracle().orc_std_encode(rgb.ctypes.data, W, H, qlum.ctypes.data, qchrom.ctypes.data, dct.ctypes.data,
                                 subsample, keep, C.byref(res))
    if rc != 0:
        raise RuntimeError("orc_std_encode failed: %d" % rc)
    out = Encoded()
    out.W8, out.H8, out.n_blocks, out.n_bits = res.W8, res.H8, res.n_blocks, res.n_bits
    out.bits = np.ctypeslib.as_array(res.bits, (res.bits_bytes,)).copy()
    units = (6 if subsample else 3) * res.n_blocks
    out.zigzag = np.ctypeslib.as_array(res.zigzag, (units, 64)).copy() if res.zigzag else None
    out.unit_bits = np.ctypeslib.as_array(res.unit_bits, (units,)).copy() if res.unit_bits else None
    oracle().orc_result_free(C.byref(res))
    return out


def oracle_std_jfif_restart(rgb, qlum, qchrom, subsample=0, interval=64):
    """Whole file of standard mode with restart markers every `interval` MCUs."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    H, W, _ = rgb.shape
    qlum = np.ascontiguousarray(qlum, np.uint32)
    qchrom = np.ascontiguousarray(qchrom, np.uint32)
    dct = np.ascontiguousarray(std_dct_table(), np.int64)
    cap = 4 * W * H * 3 + (1 << 16)
    out = np.empty(cap, np.uint8)
    n = oracle().orc_std_jfif_restart(rgb.ctypes.data, W, H, qlum.ctypes.data, qchrom.ctypes.data, dct.ctypes.data,
                                      subsample, interval, out.ctypes.data, cap)
    if n <= 0:
        raise RuntimeError("orc_std_jfif_restart failed: %d" % n)
    return out[:n].tobytes()


def ref_encode(rgb, qlum=None, qchrom=None, cds_on=True, keep=0):
    """Run the REAL reference CPU path (only where oracle/_ref is built)."""
    L = ref()
    assert L is not None, "oracle/_ref/libjpegref.so not available"
    rgb = np.ascontiguousarray(rgb, np.uint8)
    H, W, _ = rgb.shape
    if qlum is None:
        qlum = np.zeros(64, np.uint32)
        qchrom = np.zeros(64, np.uint32)
        L.ref_quant_tables(qlum.ctypes.data, qchrom.ctypes.data)
    qlum = np.ascontiguousarray(qlum, np.uint32)
    qchrom = np.ascontiguousarray(qchrom, np.uint32)
    k = (1 if keep & KEEP_U8_STAGES else 0) | (2 if keep & KEEP_DCT else 0)
    h = L.ref_run(rgb.ctypes.data, W, H, qlum.ctypes.data, qchrom.ctypes.data, int(cds_on), k)
    assert h
    out = Encoded()
    w8, h8 = C.c_size_t(), C.c_size_t()
    L.ref_dims(h, C.byref(w8), C.byref(h8))
    out.W8, out.H8 = w8.value, h8.value
    N = out.W8 * out.H8 // 64
    out.n_blocks = N
    out.n_bits = L.ref_nbits(h)
    chars = np.ctypeslib.as_array(C.cast(L.ref_bits(h), C.POINTER(C.c_uint8)), (max(out.n_bits, 1),))
    out.bit_chars = chars[:out.n_bits].copy()
    out.bits = np.packbits(out.bit_chars - ord("0"))
    out.zigzag = np.ctypeslib.as_array(L.ref_zigzag(h), (3 * N, 64)).copy()
    if keep & KEEP_U8_STAGES:
        out.csc = np.ctypeslib.as_array(L.ref_csc(h), (H, W, 3)).copy()
        out.cds = np.ctypeslib.as_array(L.ref_cds(h), (H, W, 3)).copy()
        out.padded = np.ctypeslib.as_array(L.ref_padded(h), (out.H8, out.W8, 3)).copy()
    if keep & KEEP_DCT:
        out.dct = np.ctypeslib.as_array(L.ref_dct(h), (out.H8, out.W8, 3)).copy()
    out.stage_us = [L.ref_stage_us(h)[i] for i in range(9)]
    L.ref_free(h)
    return out


def unpack_bits(packed, n_bits):
    return np.unpackbits(np.asarray(packed, np.uint8))[:n_bits]


def jfif_frame(bits, n_bits, W, H, qlum, qchrom, subsample=0):
    bits = np.ascontiguousarray(bits, np.uint8)
    cap = 2 * bits.size + 2048
    out = np.empty(cap, np.uint8)
    qlum = np.ascontiguousarray(qlum, np.uint32)
    qchrom = np.ascontiguousarray(qchrom, np.uint32)
    n = oracle().orc_jfif_frame_s(bits.ctypes.data, n_bits, W, H, qlum.ctypes.data,
                                  qchrom.ctypes.data, subsample, out.ctypes.data, cap)
    assert n > 0
    return out[:n].tobytes()


# ---------------------------------------------------------------- one-component (gray) builder
# Annex K luma tables (K.3 DC, K.5 AC).  The expected scan of an MI355_F_GRAY frame is built from the checker's luma
# rows (gray_checker_rows) with these tables: DC differences, ZRL, EOB omitted after a non-zero coefficient 63.
DC_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7,
    0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5,
    0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
    0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
    0xF9, 0xFA]


def canonical(bits, vals):
    """{symbol: (code, length)} of a BITS/HUFFVAL table (Annex C)."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


DC_TAB, AC_TAB = canonical(DC_BITS, DC_VALS), canonical(AC_BITS, AC_VALS)


def gray_entropy_code(rows):
    """Scan bits of one-component zig-zag rows [N][64] (scan order): (packed bytes, bit count)."""
    rows = np.asarray(rows, np.int64)
    codes, lens = [], []

    def put(sym_tab, sym, value, size):
        c, l = sym_tab[sym]
        v = value if value >= 0 else value + (1 << size) - 1
        codes.append((c << size) | (v & ((1 << size) - 1)))
        lens.append(l + size)

    ac = rows[:, 1:]
    nzb, nzk = np.nonzero(ac)
    bounds = np.searchsorted(nzb, np.arange(len(rows) + 1))
    nzv = ac[nzb, nzk]
    pred = 0
    for b in range(len(rows)):
        d = int(rows[b, 0]) - pred
        pred = int(rows[b, 0])
        s = abs(d).bit_length()
        put(DC_TAB, s, d, s)
        last = 0  # zig-zag position of the last coded coefficient
        for i in range(bounds[b], bounds[b + 1]):
            k, v = int(nzk[i]) + 1, int(nzv[i])
            run = k - last - 1
            while run > 15:
                put(AC_TAB, 0xF0, 0, 0)
                run -= 16
            s = abs(v).bit_length()
            put(AC_TAB, (run << 4) | s, v, s)
            last = k
        if last != 63:
            put(AC_TAB, 0x00, 0, 0)
    L = np.array(lens, np.int64)
    Cd = np.array(codes, np.int64)
    n_bits = int(L.sum())
    sym = np.repeat(np.arange(len(L)), L)
    k = np.arange(n_bits) - np.repeat(np.cumsum(L) - L, L)
    bits = ((Cd[sym] >> (L[sym] - 1 - k)) & 1).astype(np.uint8)
    return np.packbits(bits), n_bits


def jfif_gray(packed, n_bits, W, H, ql):
    """One-component baseline JFIF around a scan (the builder's container, independent of the library's)."""
    zz = zigzag_order()
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += b"\xff\xdb\x00\x43\x00" + bytes(int(ql.reshape(64)[zz[k]]) for k in range(64))
    out += b"\xff\xc0\x00\x0b\x08" + H.to_bytes(2, "big") + W.to_bytes(2, "big") + b"\x01\x01\x11\x00"
    for cls, bits, vals in ((0x00, DC_BITS, DC_VALS), (0x10, AC_BITS, AC_VALS)):
        out += b"\xff\xc4" + (3 + 16 + len(vals)).to_bytes(2, "big") + bytes([cls] + bits + vals)
    out += b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00"
    nb = (n_bits + 7) // 8
    scan = bytearray(np.asarray(packed[:nb], np.uint8).tobytes())
    if n_bits & 7:
        scan[-1] |= 0xFF >> (n_bits & 7)
    out += scan.replace(b"\xff", b"\xff\x00") + b"\xff\xd9"
    return bytes(out)


def gray_checker_rows(gray, ql, qc):
    """Luma rows of the standard-mode checker on (g,g,g): the expected coefficients of the gray frame."""
    H, W = gray.shape
    N = ((W + 7) // 8) * ((H + 7) // 8)
    o = oracle_std_encode(np.repeat(gray[:, :, None], 3, 2), ql, qc, keep=KEEP_ZIGZAG)
    return o.zigzag[:N]


# ---------------------------------------------------------------- arbitrary tables: rounding and tie mining
# (tests/test_quant_tables.py)  A quotient c/Q sits at a rounding tie when its fraction is 1/2.  The miner picks, for a
# given table, the candidate blocks whose quotient at each (component, position) lies closest to a tie on either side
# and copies them into a small frame.  Colour conversion is per pixel, performCDS works on even-aligned 2x2 quads and
# 4:2:0 chroma on whole 16x16 MCUs, so a block (MCU) copied to an aligned position keeps its transform.

def round_half_away(x):
    """C's round() of fp64 values, exactly: floor(|x|) + (fraction >= 1/2), sign restored."""
    x = np.asarray(x, np.float64)
    a = np.abs(x)
    f = np.floor(a)
    return np.copysign(f + (a - f >= 0.5), x)


def tie_distance(z):
    """| frac(|z|) - 1/2 |: how far a quotient lies from a rounding tie."""
    a = np.abs(np.asarray(z, np.float64))
    return np.abs(a - np.floor(a) - 0.5)


def to_blocks(planes, A=8):
    """(H, W, C) planes -> (C, N, A*A) blocks in scan order (block row-major), [y*A + x] inside a block."""
    H, W, C_ = planes.shape
    return planes.reshape(H // A, A, W // A, A, C_).transpose(4, 0, 2, 1, 3).reshape(C_, -1, A * A)


def strict_samples(rgb, cds_on=True):
    """Strict mode's level-shifted samples (performCSC, performCDS, -128) as (3, N, 64) fp64.  Sides must be multiples
    of 8: no mirror padding."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    H, W, _ = rgb.shape
    assert W % 8 == 0 and H % 8 == 0, (W, H)
    img = rgb.copy()
    oracle().orc_csc(img.ctypes.data, W * H)
    if cds_on:
        oracle().orc_cds(img.ctypes.data, W, H)
    return np.ascontiguousarray(to_blocks(img), np.float64) - 128.0


def strict_chain(rgb, cds_on=True):
    """The fp64 chain values of strict mode before quantisation (the oracle's in-place DCT on strict_samples):
    (3, N, 64), coefficient (u, v) at [v*8 + u]."""
    P = strict_samples(rgb, cds_on)
    oracle().orc_dct_blocks(P.ctypes.data, P.size // 64)
    return P


def strict_quantise(chain, qlum, qchrom):
    """performQuantization + zig-zag on chain values (3, N, 64): int32 rows [3N][64] in the oracle's row order.
    Defined also where the entropy stage refuses a category."""
    q = np.stack([qlum, qchrom, qchrom]).reshape(3, 1, 64).astype(np.float64)
    return round_half_away(chain / q)[:, :, zigzag_order()].reshape(-1, 64).astype(np.int32)


_INPLACE = None


def strict_exact_map():
    """The strict transform in exact arithmetic: the in-place DCT of the reference (orc_dct_block: output (u, v) is
    stored to P[v][u] before the next one is formed) is linear in the samples; returns its 64x64 matrix scaled by
    2^96 and rounded, as five balanced int64 limbs of 24 bits (entries of the product with integer samples are exact
    to 2^-84).  The cosines come from mpmath at 60 digits."""
    global _INPLACE
    if _INPLACE is None:
        import mpmath
        mpmath.mp.dps = 60
        S = 160
        cosi = [[int(mpmath.nint(mpmath.cos((2 * x + 1) * u * mpmath.pi / 16) * 2 ** 80)) for u in range(8)]
                for x in range(8)]
        a = [1 / mpmath.sqrt(2)] + [mpmath.mpf(1)] * 7
        rows = [[(1 << S) if i == j else 0 for j in range(64)] for i in range(64)]  # P[i] as a form in the samples
        for u in range(8):
            for v in range(8):
                sc = int(mpmath.nint(a[u] * a[v] / 4 * 2 ** 80))
                acc = [0] * 64
                for y in range(8):
                    for x in range(8):
                        w = cosi[x][u] * cosi[y][v]
                        if w:
                            r = rows[y * 8 + x]
                            for j in range(64):
                                acc[j] += w * r[j]
                rows[v * 8 + u] = [(t * sc) >> 240 for t in acc]
        M = [[(t + (1 << (S - 97))) >> (S - 96) for t in r] for r in rows]
        limbs = np.zeros((5, 64, 64), np.int64)
        for i in range(64):
            for j in range(64):
                t = M[i][j]
                for l in range(5):
                    d = ((t + (1 << 23)) & ((1 << 24) - 1)) - (1 << 23)
                    limbs[l, i, j] = d
                    t = (t - d) >> 24
                assert t == 0
        _INPLACE = limbs
    return _INPLACE


def strict_exact_round(samples, q):
    """round-half-away(exact in-place transform / Q) of integer-valued samples (n, 64): int64 (n, 64), natural order;
    q: (64,) natural order or (n, 64)."""
    limbs = strict_exact_map()
    p = np.asarray(samples).astype(np.int64)
    X = np.zeros(p.shape, object)
    for l in range(5):
        X = X + (p @ limbs[l].T).astype(object) * (1 << (24 * l))
    D = np.broadcast_to(np.asarray(q, np.int64), p.shape).astype(object) << 96
    A = np.abs(X)
    n = (2 * A + D) // (2 * D)
    return np.where(X < 0, -n, n).astype(np.int64)


def dct2(samples, A=8):
    """Orthonormal fp64 DCT-II of uint8 samples (..., 64) minus 128: (..., 64), coefficient (u, v) at [v*8 + u]."""
    k = np.arange(8)
    C_ = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) / 2  # [u][x]
    C_[0] /= np.sqrt(2)
    s = np.asarray(samples, np.float64).reshape(samples.shape[:-1] + (8, 8)) - 128.0
    return (C_ @ s @ C_.T).reshape(samples.shape)


def tie_pool(W=2048, H=2048, seed=20261015):
    """The candidate pool of the tie miner: one RGB frame of (W/8)(H/8) blocks, mixed per 16x16 MCU from LCG noise,
    smooth waves, two-level blocks, saturated pixels (0, 1, 254, 255) and constant 8x8 blocks."""
    rng = np.random.default_rng(seed)
    mh, mw = H // 16, W // 16
    kind = np.kron(rng.integers(0, 5, (mh, mw)), np.ones((16, 16), np.int64))[..., None]
    noise = lcg_frame(W, H, seed & 0xFFFF).astype(np.float64)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)

    def per_mcu(lo, hi, ch=3):
        return np.kron(rng.uniform(lo, hi, (mh, mw, ch)), np.ones((16, 16, 1)))

    fx, fy, ph, amp, mid = per_mcu(0, 1.6), per_mcu(0, 1.6), per_mcu(0, 6.3), per_mcu(10, 130), per_mcu(40, 215)
    smooth = mid + amp * np.cos(fx * x[..., None] + fy * y[..., None] + ph) + rng.normal(0, 1.5, (H, W, 3))
    bh, bw = H // 8, W // 8
    c0 = np.kron(rng.integers(0, 256, (bh, bw, 3)), np.ones((8, 8, 1)))
    c1 = np.kron(rng.integers(0, 256, (bh, bw, 3)), np.ones((8, 8, 1)))
    split = rng.random((H, W, 1)) < np.kron(rng.random((bh, bw, 1)), np.ones((8, 8, 1)))
    two = np.where(split, c0, c1)
    sat = np.array([0, 1, 254, 255])[rng.integers(0, 4, (H, W, 3))]
    const = c0
    out = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [noise, smooth, two, sat], const)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


class TieMiner:
    """Tie mining over one candidate pool (tie_pool).  Value sets, each (components, 64, candidates):
      ("strict", cds) -- the oracle's fp64 chain values (one run with KEEP_DCT), candidates = 8x8 blocks
      "std"           -- fp64 DCT-II of standard mode's samples (std_csc), 8x8 blocks
      "gray"          -- the luma of "std": the gray frames are std_csc's luma bytes
      "420"           -- per 16x16 MCU: the four luma blocks and the two 4:2:0 chroma blocks (std_chroma420)
    frame(...) returns the mined frame and the candidate ids it is made of (block b of the frame = candidate ids[b])."""

    def __init__(self, pool=None):
        self.pool = tie_pool() if pool is None else pool
        self.H, self.W, _ = self.pool.shape
        self._values, self._picked, self._blocks = {}, {}, {}
        self.gray_pool = std_csc(self.pool)[..., 0].astype(np.uint8)

    def values(self, key):
        if key not in self._values:
            if key[0] == "strict":
                q = np.full(64, 255, np.uint32)  # (quotients of at most 5: no category is refused)
                o = oracle_encode(self.pool, q, q, key[1], KEEP_DCT)
                v = to_blocks(o.dct)
            elif key == "std":
                v = dct2(to_blocks(std_csc(self.pool)))
            elif key == "gray":
                v = self.values("std")[:1].transpose(0, 2, 1)
            else:
                luma = to_blocks(std_csc(self.pool)[..., :1], 16)[0].reshape(-1, 2, 8, 2, 8)
                luma = luma.transpose(0, 1, 3, 2, 4).reshape(-1, 4, 64).transpose(1, 0, 2)  # [k = 2 row + col][mcu]
                ch = to_blocks(std_chroma420(self.pool), 8)
                v = dct2(np.concatenate([luma, ch]))
            self._values[key] = np.ascontiguousarray(v.transpose(0, 2, 1))
        return self._values[key]

    def pick(self, key, Q, k=2, stride=1):
        """Candidate ids: per (component, position) the k nearest below a tie and the k nearest at or above it.
        Q: (components, 64) divisors, natural order."""
        V = self.values(key)
        nc = V.shape[0]
        out, todo = {}, []
        for c in range(nc):
            for p in range(64):
                ck = (key, c, p, int(Q[c][p]), k, stride)
                if ck in self._picked:
                    out[c, p] = self._picked[ck]
                else:
                    todo.append((c, p))
        if todo:
            cs, ps = np.array(todo).T
            z = np.abs(V[cs, ps, ::stride]) / np.asarray(Q, np.float64)[cs, ps][:, None]
            f = z - np.floor(z)
            sel = []
            for d in (np.where(f < 0.5, 0.5 - f, np.inf), np.where(f >= 0.5, f - 0.5, np.inf)):
                i = np.argpartition(d, k, axis=1)[:, :k]
                sel.append(np.where(np.isfinite(np.take_along_axis(d, i, 1)), i * stride, -1))
            sel = np.concatenate(sel, 1)
            for j, (c, p) in enumerate(todo):
                ids = sel[j][sel[j] >= 0]
                self._picked[(key, c, p, int(Q[c][p]), k, stride)] = out[c, p] = ids
        return np.unique(np.concatenate(list(out.values())))

    def blocks(self, ids, A=8, gray=False):
        """Candidates ids as (n, A, A, 3) RGB blocks ((n, A, A) gray)."""
        src = self.gray_pool[..., None] if gray else self.pool
        if (A, gray) not in self._blocks:
            H, W, C_ = src.shape
            self._blocks[A, gray] = src.reshape(H // A, A, W // A, A, C_).transpose(0, 2, 1, 3, 4).reshape(-1, A, A, C_)
        b = self._blocks[A, gray][np.asarray(ids, np.int64)]
        return b[..., 0] if gray else b

    @staticmethod
    def assemble(blocks, cols=32):
        """Blocks (n, A, A[, 3]) laid out row-major, `cols` to a row; the last row is filled up with copies of the
        first block."""
        n, A = len(blocks), blocks.shape[1]
        cols = min(cols, n)
        rows = -(-n // cols)
        blocks = np.concatenate([blocks, np.repeat(blocks[:1], rows * cols - n, 0)])
        f = blocks.reshape((rows, cols, A, A, -1)).transpose(0, 2, 1, 3, 4).reshape(rows * A, cols * A, -1)
        return np.ascontiguousarray(f[..., 0] if blocks.ndim == 3 else f)

    def strict(self, ql, qc, cds_on=True, k=2, stride=1, forge=True):
        """Mined frame of strict mode and the chain values the oracle gives its blocks (3, N, 64), taken from the pool
        run.  With forge: one block more whose luma coefficient at the table's smallest divisor off the column u = 0 lies within about
        1e-9 of a tie (forge_luma_tie), when that divisor admits ties (<= 2000)."""
        key = ("strict", bool(cds_on))
        ids = self.pick(key, [ql, qc, qc], k, stride)
        blocks = self.blocks(ids)
        vals = self.values(key)[:, :, ids].transpose(0, 2, 1)
        if forge:
            # (the column u = 0 is left out: its rows weigh each sample row alike, too few sums for the search)
            r = min((int(ql[p]), p) for p in range(64) if p % 8)[1]
            Q = int(ql[r])
            if Q <= 2000:
                b = self.forge_luma_tie(r, Q)
                blocks = np.concatenate([blocks, b[None]])
                vals = np.concatenate([vals, strict_chain(b, cds_on)], 1)
        f = self.assemble(blocks)
        n = len(blocks)
        N = f.shape[0] * f.shape[1] // 64
        vals = np.concatenate([vals, np.repeat(vals[:, :1], N - n, 1)], 1)
        return f, vals

    def forge_luma_tie(self, r, Q):
        """An 8x8 RGB block whose strict luma coefficient at natural position r has chain value within about 1e-9 of a
        tie Q (k + 1/2): the pool's nearest candidate, with three luma samples of each half of the block moved by one
        level (meet in the middle over the ~4e4 x 4e4 combinations, on the exact transform's matrix).  Such a value
        leaves the screened quantiser's second look undecided: the exact chain must decide it."""
        ck = ("forge", r, Q)
        if ck in self._picked:
            return self._picked[ck]
        inv = _strict_luma_inverse()
        V = self.values(("strict", True))[0, r]
        d = tie_distance(V / Q)
        best = None
        for b in np.argsort(d)[:8]:
            blk = self.blocks([b])[0]
            y = (strict_samples(blk, False)[0, 0] + 128).astype(np.int64)
            if y.min() < 1 or y.max() > 254:
                continue
            best = (blk, y, float(V[b]))
            break
        assert best is not None
        blk, y, c0 = best
        m = _strict_map_float()[r]
        from itertools import combinations
        halves = []
        for lo in (0, 32):
            idx = np.array(list(combinations(range(lo, lo + 32), 3)))
            sg = np.array([[a, b_, c] for a in (-1, 1) for b_ in (-1, 1) for c in (-1, 1)])
            I = np.repeat(idx, 8, 0)
            S = np.tile(sg, (len(idx), 1))
            halves.append((I, S, (S * m[I]).sum(1)))
        (I1, S1, a1), (I2, S2, a2) = halves
        A_ = np.mod((c0 + a1) / Q, 1.0)
        B_ = np.mod(a2 / Q, 1.0)
        order = np.argsort(B_)
        Bs = B_[order]
        t = np.mod(0.5 - A_, 1.0)
        j = np.searchsorted(Bs, t) % len(Bs)
        cand = []
        for jj in (j, (j - 1) % len(Bs)):
            dd = np.abs(Bs[jj] - t)
            cand.append((np.minimum(dd, 1 - dd), jj))
        dist = np.minimum(cand[0][0], cand[1][0])
        i = int(np.argmin(dist))
        jj = int(cand[0][1][i] if cand[0][0][i] <= cand[1][0][i] else cand[1][1][i])
        k2 = int(order[jj])
        y = y.copy()
        y[I1[i]] += S1[i]
        y[I2[k2]] += S2[k2]
        out = blk.reshape(64, 3).copy()
        for s in np.concatenate([I1[i], I2[k2]]):
            out[s] = inv[y[s]]
        out = out.reshape(8, 8, 3)
        self._picked[ck] = out
        return out

    def standard(self, ql, qc, k=2, stride=1):
        return self.assemble(self.blocks(self.pick("std", [ql, qc, qc], k, stride)))

    def gray(self, ql, k=2, stride=1):
        return self.assemble(self.blocks(self.pick("gray", [ql], k, stride), gray=True))

    def s420(self, ql, qc, k=2, stride=1):
        return self.assemble(self.blocks(self.pick("420", [ql] * 4 + [qc, qc], k, stride), A=16), cols=16)


_LUMA_INV, _MAP_FLOAT = None, None


def _strict_luma_inverse():
    """For each strict luma level Y, one RGB pixel that performCSC turns into Y."""
    global _LUMA_INV
    if _LUMA_INV is None:
        rgb = np.stack(np.meshgrid(np.arange(256), np.arange(256), np.arange(0, 256, 5), indexing="ij"), -1)
        rgb = np.ascontiguousarray(rgb.reshape(-1, 3), np.uint8)
        img = rgb.copy()
        oracle().orc_csc(img.ctypes.data, len(img))
        inv = np.zeros((256, 3), np.uint8)
        seen = np.zeros(256, bool)
        inv[img[::-1, 0]] = rgb[::-1]
        seen[img[:, 0]] = True
        assert seen.all()
        _LUMA_INV = inv
    return _LUMA_INV


def _strict_map_float():
    global _MAP_FLOAT
    if _MAP_FLOAT is None:
        L = strict_exact_map().astype(np.float64)
        _MAP_FLOAT = sum(L[l] * 2.0 ** (24 * l - 96) for l in range(5))
    return _MAP_FLOAT
