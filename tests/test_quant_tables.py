"""The fused encoders under arbitrary and extreme quantisation tables.

mi355_jpeg_set_quant takes any table with entries 1..65535, and the tables are the one caller input that reshapes the
fused path's internal constants (the first- and second-look thresholds and the fp32 scale per table position, the
integer DC quotient).  Strict mode promises the reference's bits for every such table; standard and gray mode promise
the quotient contract of include/mi355_jpeg.h.  The tables here are constant, huge, "spike" (255 except a 1 at one
position), random, transposed and swapped -- never only IJG scaling -- and the inputs are mined for each table: blocks
of a large candidate pool whose quotients lie closest to a rounding tie at every (component, position)
(oracle_lib.TieMiner), plus, in strict mode, one block forged to sit within ~1e-9 of a tie, which the screened
quantiser cannot decide without the exact chain."""
import importlib
import io

import numpy as np
import pytest

import oracle_lib as ol

PIL = pytest.importorskip("PIL.Image")
jpeg_mod = importlib.import_module("jpeg-encoder-opencl_amd")
F_CDS, F_STD, F_420, F_RESTART, F_GRAY = 1, 2, 4, 8, 16
GRAY = F_STD | F_GRAY
ZZ = ol.zigzag_order()
KEEP = ol.KEEP_ZIGZAG | ol.KEEP_UNIT_BITS


# ---------------------------------------------------------------- the table families
def _u32(*a):
    return tuple(np.ascontiguousarray(np.broadcast_to(np.asarray(x), (64,)), np.uint32).copy() for x in a)


def constant_tables():
    return {"const%d" % q: _u32(q, 256 - q) for q in range(1, 256)}


LARGE = [256, 257, 1000, 4095, 4096, 32767, 32768, 65534, 65535]


def large_tables():
    return {"large%d" % q: _u32(q, LARGE[(i + 4) % len(LARGE)]) for i, q in enumerate(LARGE)}


def spike_tables():
    out = {}
    for p in range(64):
        t = np.full(64, 255, np.uint32)
        t[p] = 1
        out["spike_lum%d" % p] = _u32(t, 255)
        out["spike_chr%d" % p] = _u32(255, t)
    return out


def random_tables():
    rng = np.random.default_rng(20261015)
    out = {}
    for i in range(2):
        out["uniform%d" % i] = _u32(rng.integers(1, 256, 64), rng.integers(1, 256, 64))
    for i in range(2):
        out["loguniform%d" % i] = _u32(*np.rint(np.exp(rng.uniform(0, np.log(65535), (2, 64)))).clip(1, 65535))
    for q in (50, 90):
        ql, qc = ol.quant_tables(q)
        out["transposed_q%d" % q] = _u32(ql.reshape(8, 8).T.reshape(64), qc.reshape(8, 8).T.reshape(64))
    for q in (50, 75):
        ql, qc = ol.quant_tables(q)
        out["swapped_q%d" % q] = _u32(qc, ql)
    return out


FAMILIES = {"constant": constant_tables, "large": large_tables, "spike": spike_tables, "random": random_tables}


def small_tables():
    """Tables with every entry <= 255 (a file can carry them): a spread over the families."""
    t = {k: v for k, v in constant_tables().items() if int(k[5:]) in (1, 2, 3, 7, 16, 64, 127, 200, 255)}
    t.update({k: v for k, v in spike_tables().items() if int(k[9:]) % 9 in (0, 4)})
    t.update({k: v for k, v in random_tables().items() if "loguniform" not in k})
    return t


@pytest.fixture(scope="module")
def miner():
    return ol.TieMiner()


def qnat(ql, qc):
    """(3, 64) divisors per component, natural order."""
    return np.stack([ql, qc, qc]).astype(np.float64)


# ---------------------------------------------------------------- CPU: the miner itself
SPREAD = ["const1", "const2", "const7", "const16", "const100", "const255", "large256", "large1000",
          "spike_lum9", "spike_chr40", "uniform0", "transposed_q90", "swapped_q50"]


def _table(name):
    for fam in FAMILIES.values():
        t = fam()
        if name in t:
            return t[name]
    raise KeyError(name)


@pytest.mark.parametrize("cds", [True, False], ids=["cds", "nocds"])
def test_oracle_reproduces_the_mined_chain_values(miner, cds):
    """The oracle run on an assembled frame gives its blocks, bit for bit, the chain values mined from the pool run;
    strict_quantise of them is the oracle's zig-zag output."""
    for name in ("const7", "spike_chr40", "uniform0", "large1000"):
        ql, qc = _table(name)
        f, vals = miner.strict(ql, qc, cds)
        o = ol.oracle_encode(f, ql, qc, cds, ol.KEEP_DCT | ol.KEEP_ZIGZAG)
        assert np.array_equal(ol.to_blocks(o.dct), vals), name
        assert np.array_equal(ol.strict_chain(f, cds), vals), name
        assert np.array_equal(o.zigzag, ol.strict_quantise(vals, ql, qc)), name


def test_standard_miners_keep_their_samples(miner):
    """Moved blocks (4:4:4, gray) and MCUs (4:2:0) keep the samples they had in the pool."""
    ql, qc = _table("uniform1")
    f = miner.standard(ql, qc)
    ids = miner.pick("std", [ql, qc, qc])
    want = miner.values("std")[:, :, ids].transpose(0, 2, 1)
    got = ol.dct2(ol.to_blocks(ol.std_csc(f)))[:, :len(ids)]
    assert np.array_equal(got, want)
    g = miner.gray(ql)
    ids = miner.pick("gray", [ql])
    assert np.array_equal(ol.dct2(ol.to_blocks(g[..., None]))[:, :len(ids)], miner.values("gray")[:, :, ids].transpose(0, 2, 1))
    f = miner.s420(ql, qc)
    ids = miner.pick("420", [ql] * 4 + [qc, qc])
    ch = ol.to_blocks(ol.std_chroma420(f), 8)[:, :len(ids)]
    assert np.array_equal(ol.dct2(ch), miner.values("420")[4:, :, ids].transpose(0, 2, 1))


@pytest.mark.parametrize("name", SPREAD)
def test_mined_frames_sit_on_ties_and_defeat_naive_rounding(miner, name):
    """The mined frames put coefficients within 1e-9 of a tie, and two naive quantisers get some of them wrong: the
    exact transform rounded exactly (the chain's own rounding decides a tie), and the chain value divided in fp32."""
    ql, qc = _table(name)
    for cds in (True, False):
        f, vals = miner.strict(ql, qc, cds)
        q = qnat(ql, qc)[:, None, :]
        assert (ol.tie_distance(vals / q) < 1e-9).sum() > 0, (name, cds)
        want = ol.round_half_away(vals / q)
        S = ol.strict_samples(f, cds)
        exact = np.stack([ol.strict_exact_round(S[c], q[c, 0].astype(np.int64)) for c in range(3)])
        f32 = ol.round_half_away((vals.astype(np.float32) / q.astype(np.float32)).astype(np.float64))
        assert (exact != want).sum() > 0, (name, cds)
        assert (f32 != want).sum() > 0, (name, cds)
        assert np.abs(exact - want).max() <= 1 and np.abs(f32 - want).max() <= 1


def test_forged_block_is_closer_to_a_tie_than_the_screen_can_decide(miner):
    """The forged luma coefficient lies within 2^-27 (the second look's margin) of a tie, for small divisors."""
    for Q in (1, 2, 5, 16):
        for r in (1, 9, 27, 63):
            b = miner.forge_luma_tie(r, Q)
            c = ol.strict_chain(b, True)[0, 0, r]
            assert abs(abs(c) / Q - np.floor(abs(c) / Q) - 0.5) * Q < 2.0 ** -27, (Q, r, c)


def test_standard_mined_frames_come_near_the_contract_window(miner):
    """4:4:4, 4:2:0 and gray mined frames put quotients inside the 2e-3 window of the contract and just outside it."""
    for name in ("const3", "uniform0", "spike_lum20"):
        ql, qc = _table(name)
        f = miner.standard(ql, qc)
        d = ol.tie_distance(ol.dct2(ol.to_blocks(ol.std_csc(f))) / qnat(ql, qc)[:, None, :])
        assert (d < 2e-3).sum() > 0 and ((d >= 2e-3) & (d < 1e-2)).sum() > 0, name


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def qenc():
    e = jpeg_mod.Encoder(0)  # a context of its own: no table leaks into other modules
    yield e
    e.close()


def _strict_case(enc, jpeg, ql, qc, cds, rgb, chain, unit_bits, tag):
    flags = F_CDS if cds else 0
    want = ol.strict_quantise(chain, ql, qc)
    got = enc.probe_coefficients(rgb, flags).astype(np.int32)
    assert np.array_equal(got, want), (tag, int((got != want).sum()))
    try:
        o = ol.oracle_encode(rgb, ql, qc, cds, KEEP)
    except RuntimeError:  # a category outside the reference's tables: both sides refuse
        with pytest.raises(jpeg.JpegError) as ei:
            enc.encode_scan(rgb, flags)
        assert ei.value.status == jpeg.E_CATEGORY, tag
        return
    assert np.array_equal(o.zigzag, want), tag
    bits, nb = enc.encode_scan(rgb, flags)
    assert nb[0] == o.n_bits and np.array_equal(bits[0], o.bits), tag
    if unit_bits:
        assert np.array_equal(enc.probe_unit_bits(rgb, flags), o.unit_bits), tag


LCG = ol.lcg_frame(96, 64, 77)
_LCG_CHAIN = {}


@pytest.mark.gpu
@pytest.mark.parametrize("cds", [True, False], ids=["cds", "nocds"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_strict_bits_under_every_table_shape(jpeg, qenc, miner, family, cds):
    """probe_coefficients = the oracle's quotients, scan bits (and, for some tables, per-unit bits) = the oracle's, on
    each table's mined frame and on an LCG frame; the mined frames reach the second look and the exact chain."""
    if cds not in _LCG_CHAIN:
        _LCG_CHAIN[cds] = ol.strict_chain(LCG, cds)
    tables = FAMILIES[family]()
    qenc.screen_stats(reset=True)
    looks = exact = 0
    for i, (name, (ql, qc)) in enumerate(tables.items()):
        qenc.set_quant(ql, qc)
        assert all(np.array_equal(a, b) for a, b in zip(qenc.get_quant(), (ql, qc)))
        # the 255 constant tables are mined from every 8th candidate (forging where Q = 1 mod 16)
        stride, forge = (8, (i % 16) == 0) if family == "constant" else (1, True)
        f, vals = miner.strict(ql, qc, cds, stride=stride, forge=forge)
        qenc.screen_stats(reset=True)
        _strict_case(qenc, jpeg, ql, qc, cds, f, vals, i % 8 == 0, (family, name, cds))
        lk, ex = qenc.screen_stats(reset=True)
        looks, exact = looks + lk, exact + ex
        _strict_case(qenc, jpeg, ql, qc, cds, LCG, _LCG_CHAIN[cds], i % 8 == 1, (family, name, cds, "lcg"))
    print("screen_stats of the mined frames, %s tables, %s: second looks %d, exact units %d"
          % (family, "cds" if cds else "nocds", looks, exact))
    if family != "large":  # (no divisor of 256 and more admits a tie the second look cannot decide)
        assert looks > 0 and exact > 0, (family, looks, exact)


def _std_contract(rows, dct_nat, qn, counts):
    """Each coefficient = round-half-away(DCT/Q) except within 2e-3 of a tie, where it may be the other neighbour.
    rows: (n, 64) zig-zag; dct_nat: (n, 64) natural order; qn: (n, 64) or (64,) natural order."""
    z = dct_nat[:, ZZ] / np.broadcast_to(qn, dct_nat.shape)[:, ZZ]
    want = ol.round_half_away(z)
    d = ol.tie_distance(z)
    bad = rows != want
    assert np.all(np.abs(rows - want)[bad] == 1), int(bad.sum())
    assert np.all(d[bad] < 2e-3), float(d[bad].max())
    counts[0] += int((d < 2e-3).sum())
    counts[1] += int(((d >= 2e-3) & (d < 4e-3)).sum())


def _std_tables():
    t = small_tables()
    t.update(large_tables())  # (scans only)
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["444", "420", "gray"])
def test_standard_checker_parity_and_contract(jpeg, qenc, miner, layout):
    counts = [0, 0]
    for name, (ql, qc) in _std_tables().items():
        qenc.set_quant(ql, qc)
        if layout == "444":
            f = miner.standard(ql, qc)
            o = ol.oracle_std_encode(f, ql, qc, KEEP)
            rows = qenc.probe_coefficients(f, F_STD).astype(np.int32)
            bits, nb = qenc.encode_scan(f, F_STD)
            N = rows.shape[0] // 3
            dct = ol.dct2(ol.to_blocks(qenc.probe_samples(f, F_STD)))
            for c in range(3):
                _std_contract(rows[c * N:(c + 1) * N], dct[c], (ql if c == 0 else qc).astype(np.float64), counts)
        elif layout == "420":
            f = miner.s420(ql, qc)
            o = ol.oracle_std_encode(f, ql, qc, KEEP, subsample=1)
            rows = qenc.probe_coefficients(f, F_STD | F_420).astype(np.int32)
            bits, nb = qenc.encode_scan(f, F_STD | F_420)
            M = rows.shape[0] // 6
            luma = ol.to_blocks(ol.std_csc(f)[..., :1], 16)[0].reshape(-1, 2, 8, 2, 8).transpose(0, 1, 3, 2, 4)
            _std_contract(rows[:4 * M], ol.dct2(luma.reshape(-1, 64)), ql.astype(np.float64), counts)
            ch = ol.dct2(ol.to_blocks(ol.std_chroma420(f), 8))
            for c in range(2):
                _std_contract(rows[(4 + c) * M:(5 + c) * M], ch[c], qc.astype(np.float64), counts)
        else:
            f = miner.gray(ql)
            o = ol.Encoded()
            o.zigzag = ol.gray_checker_rows(f, ql, qc)
            o.bits, o.n_bits = ol.gray_entropy_code(o.zigzag)
            rows = qenc.probe_coefficients(f, GRAY).astype(np.int32)
            bits, nb = qenc.encode_scan(f, GRAY)
            dct = ol.dct2(ol.to_blocks(qenc.probe_samples(f, GRAY)[..., None]))
            _std_contract(rows, dct[0], ql.astype(np.float64), counts)
        assert np.array_equal(rows, o.zigzag), (layout, name)
        assert nb[0] == o.n_bits and np.array_equal(bits[0], o.bits), (layout, name)
    print("standard %s: quotients within 2e-3 of a tie %d, within 2e-3..4e-3 %d" % (layout, counts[0], counts[1]))
    assert counts[0] > 0 and counts[1] > 0


@pytest.mark.gpu
def test_gray_ignores_the_chroma_table(qenc, miner):
    ql, qc = _table("uniform0")
    f = miner.gray(ql)
    out = []
    for chroma in (qc, np.full(64, 1, np.uint32), np.full(64, 65535, np.uint32)):
        qenc.set_quant(ql, chroma)
        out.append(qenc.encode_scan(f, GRAY))
    for bits, nb in out[1:]:
        assert nb == out[0][1] and np.array_equal(bits[0], out[0][0][0])


def _psnr(a, b):
    mse = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()
    return 10 * np.log10(255.0 ** 2 / mse)


def _smooth(W, H, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([127 + 120 * np.sin(x / 37.0 + seed) * np.cos(y / 23.0),
                    127 + 100 * np.cos(x / 51.0) * np.cos(y / 17.0 + 1),
                    (x * 255 // max(W - 1, 1) + y * 255 // max(H - 1, 1)) / 2], -1)
    return np.clip(img + rng.normal(0, 3, img.shape), 0, 255).astype(np.uint8)


def _pil_roundtrip(img, tables, subsample=0):
    buf = io.BytesIO()
    kw = {} if img.ndim == 2 else {"subsampling": 2 if subsample else 0}
    PIL.fromarray(img).save(buf, "JPEG", qtables=[[int(v) for v in t] for t in tables], **kw)
    return _decode(buf.getvalue(), img.ndim == 2)


def _decode(data, gray):
    im = PIL.open(io.BytesIO(data))
    return np.asarray(im if gray else im.convert("RGB"))


def test_custom_table_files_decode_like_an_independent_encoder():
    """The checker's files under a random table (all three layouts) decode in Pillow to the picture Pillow's own file
    with the same tables gives (the GPU's files are byte-equal to these: test_jfif_with_custom_tables)."""
    ql, qc = _table("uniform1")
    rgb = _smooth(333, 201, 4)
    gray = ol.std_csc(rgb)[..., 0].astype(np.uint8)
    for ss in (0, 1):
        o = ol.oracle_std_encode(rgb, ql, qc, subsample=ss)
        ours = _decode(ol.jfif_frame(o.bits, o.n_bits, 333, 201, ql, qc, subsample=ss), False)
        theirs = _pil_roundtrip(rgb, (ql, qc), ss)
        assert _psnr(ours, theirs) > 30.0 and abs(_psnr(ours, rgb) - _psnr(theirs, rgb)) < 0.1, ss
    packed, n_bits = ol.gray_entropy_code(ol.gray_checker_rows(gray, ql, qc))
    ours = _decode(ol.jfif_gray(packed, n_bits, 333, 201, ql), True)
    theirs = _pil_roundtrip(gray, (ql,))
    assert _psnr(ours, theirs) > 30.0 and abs(_psnr(ours, gray) - _psnr(theirs, gray)) < 0.1


@pytest.mark.gpu
def test_jfif_with_custom_tables(jpeg, qenc):
    """encode_jfif under a random table <= 255 is byte-equal to the checker's file in all three layouts (this pins the
    DQT zig-zag order of a table that is not an IJG table), with restart intervals too; an entry above 255 gives
    E_TABLE from encode_jfif and wrap_jfif, but not from encode_scan."""
    ql, qc = _table("uniform1")
    qenc.set_quant(ql, qc)
    rgb = _smooth(333, 201, 4)
    gray = ol.std_csc(rgb)[..., 0].astype(np.uint8)
    for ss, flags in ((0, F_STD), (1, F_STD | F_420)):
        o = ol.oracle_std_encode(rgb, ql, qc, subsample=ss)
        assert qenc.encode_jfif(rgb, flags) == ol.jfif_frame(o.bits, o.n_bits, 333, 201, ql, qc, subsample=ss), ss
        assert qenc.encode_jfif(rgb, flags | F_RESTART) == ol.oracle_std_jfif_restart(rgb, ql, qc, subsample=ss), ss
    packed, n_bits = ol.gray_entropy_code(ol.gray_checker_rows(gray, ql, qc))
    assert qenc.encode_jfif(gray, GRAY) == ol.jfif_gray(packed, n_bits, 333, 201, ql)
    for big in (_u32(ql, np.where(np.arange(64) == 17, 256, qc)), _u32(65535, qc)):
        qenc.set_quant(*big)
        for x, flags in ((rgb, F_STD), (rgb, F_STD | F_420), (gray, GRAY)):
            bits, nb = qenc.encode_scan(x, flags)
            if flags == F_STD:
                o = ol.oracle_std_encode(x, *big)
                assert nb[0] == o.n_bits and np.array_equal(bits[0], o.bits)
            for call in (lambda: qenc.encode_jfif(x, flags), lambda: qenc.wrap_jfif(bits[0], nb[0], 333, 201, flags)):
                with pytest.raises(jpeg.JpegError) as ei:
                    call()
                assert ei.value.status == jpeg.E_TABLE, flags


# ---------------------------------------------------------------- GPU: entry points and table state
@pytest.mark.gpu
def test_refused_tables_leave_the_old_ones_in_force(jpeg, qenc):
    ql, qc = _table("uniform0")
    rgb = ol.lcg_frame(64, 48, 5)
    want = ol.oracle_encode(rgb, ql, qc, True)
    bad = [_u32(np.where(np.arange(64) == 5, 0, ql), qc), _u32(np.where(np.arange(64) == 63, 65536, ql), qc),
           _u32(ql, np.where(np.arange(64) == 30, 0, qc)), _u32(ql, np.where(np.arange(64) == 0, 65536, qc))]
    qenc.set_quant(ql, qc)
    for t in bad:
        with pytest.raises(jpeg.JpegError) as ei:
            qenc.set_quant(*t)
        assert ei.value.status == jpeg.E_TABLE
        got = qenc.get_quant()
        assert np.array_equal(got[0], ql) and np.array_equal(got[1], qc)
        bits, nb = qenc.encode_scan(rgb)
        assert nb[0] == want.n_bits and np.array_equal(bits[0], want.bits)
    pool = jpeg_mod.Pool([0, 0])
    try:
        pool.set_quant(ql, qc)
        for t in bad:
            with pytest.raises(jpeg.JpegError) as ei:
                pool.set_quant(*t)
            assert ei.value.status == jpeg.E_TABLE
            out, bits, _ = pool.encode(np.stack([rgb, rgb]))
            for f in range(2):
                assert bits[f] == want.n_bits and np.array_equal(out[f, :(bits[f] + 7) // 8], want.bits)
    finally:
        pool.close()


@pytest.mark.gpu
def test_one_table_through_every_path(jpeg, miner):
    """One random table: a device batch split into several parts on a torch stream, the pool (RGB and F_GRAY) and the
    host entry point all give the oracle's or the checker's bits."""
    import torch
    ql, qc = _table("uniform1")
    e2 = jpeg_mod.Encoder(0)
    try:
        e2.set_quant(ql, qc)
        W, H, n = 1920, 1080, 128
        dev = torch.device("cuda", 0)
        d_rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
        e2.synth_lcg_device(d_rgb.data_ptr(), W * H * 3, n, 300)
        cap = 2 << 20
        d_out = torch.zeros((n, cap), dtype=torch.uint8, device=dev)
        d_bits = torch.zeros(n, dtype=torch.int64, device=dev)
        s = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        e2.encode_scan_device(d_rgb.data_ptr(), W, H, n, d_out.data_ptr(), cap, d_bits.data_ptr(), stream=s.cuda_stream)
        e2.sync(s.cuda_stream)
        assert e2.last_call_parts() > 1
        for f in (0, n // 2, n - 1):
            o = ol.oracle_encode(d_rgb[f].cpu().numpy(), ql, qc, True)
            assert int(d_bits[f]) == o.n_bits and np.array_equal(d_out[f, :(o.n_bits + 7) // 8].cpu().numpy(), o.bits), f
        del d_rgb, d_out, d_bits
        frames = np.stack([miner.strict(ql, qc, True)[0]] * 2 + [ol.lcg_frame(256, 192, 9)])
        want = [ol.oracle_encode(x, ql, qc, True) for x in frames]
        bits, nb = e2.encode_scan(frames)
        assert nb == [o.n_bits for o in want] and all(np.array_equal(b, o.bits) for b, o in zip(bits, want))
        gray = np.stack([miner.gray(ql)] * 3)
        rows = ol.gray_checker_rows(gray[0], ql, qc)
        gpacked, gbits = ol.gray_entropy_code(rows)
        pool = jpeg_mod.Pool([0, 0])
        try:
            pool.set_quant(ql, qc)
            out, pb, _ = pool.encode(frames)
            for f in range(3):
                assert pb[f] == want[f].n_bits and np.array_equal(out[f, :(pb[f] + 7) // 8], want[f].bits), f
            out, pb, _ = pool.encode(gray, GRAY)
            for f in range(3):
                assert pb[f] == gbits and np.array_equal(out[f, :(gbits + 7) // 8], gpacked), f
        finally:
            pool.close()
    finally:
        e2.close()


@pytest.mark.gpu
def test_switching_custom_tables_between_calls(qenc, miner):
    """Two custom tables alternated over successive calls on one context: each call uses its own."""
    tabs = [_table("uniform0"), _table("spike_lum9")]
    frames = [miner.strict(ql, qc, True)[0] for ql, qc in tabs]
    want = {(t, f): ol.oracle_encode(frames[f], *tabs[t], True) for t in range(2) for f in range(2)}
    for step in range(6):
        t = step % 2
        qenc.set_quant(*tabs[t])
        for f in range(2):
            bits, nb = qenc.encode_scan(frames[f])
            o = want[t, f]
            assert nb[0] == o.n_bits and np.array_equal(bits[0], o.bits), (step, f)
