"""NumPy restatement of the baseline-JPEG encoder of include/avhot.h (av_jpeg_encode_header / av_jpeg_encode): libjpeg's default
compress path in 32-bit integers -- colour conversion, edge replication and chroma downsampling in libjpeg's order, the "islow"
forward DCT, quantisation, dummy blocks, the Annex K Huffman coding with restart intervals and byte stuffing, and the frame layout
libjpeg writes.  tests/golden/mjpeg_encode.npz (Pillow's bytes) pins it byte for byte; the library is then compared with it.  The
coefficient stages are vectorised; the Huffman coding is plain Python."""
import numpy as np

from tests import jpeg_ref as jr

SUBSAMPLING = {"444": (1, 1), "422": (2, 1), "420": (2, 2)}
EFULL = 64

# ITU-T T.81 Annex K.1, natural order
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80,
                      62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98,
                      112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99,
                        99] + [99] * 32)


def _fix(x):
    return int(x * 65536 + 0.5)


def quant_tables(quality):
    """-> uint8 [2, 64], natural order: luminance, chrominance"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality %r" % (quality,))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((b * scale + 50) // 100, 1, 255) for b in (BASE_LUMA, BASE_CHROMA)]).astype(np.uint8)


def descriptor(h, w, quality, subsampling):
    """What jpeg_ref.geometry / jpeg_ref.pixels need of a frame this encoder writes."""
    hs, vs = SUBSAMPLING[subsampling]
    qt = np.zeros((4, 64), np.uint8)
    qt[:2] = quant_tables(quality)
    return dict(width=w, height=h, ncomp=3, hs=hs, vs=vs, tq=[0, 1, 1, 0], td=[0, 1, 1, 0], ta=[0, 1, 1, 0], qt=qt)


def interval_of(g, restart_mcus):
    """MCUs per restart interval: -1 is one MCU row, 0 none."""
    if restart_mcus == -1:
        return g["mcus_x"]
    if not 0 <= restart_mcus <= 65535:
        raise ValueError("restart_mcus %r" % (restart_mcus,))
    return int(restart_mcus)


def _fdct8(x, first):
    """jfdctint along the last axis; x int32 [..., 8]"""
    c = np.int32
    d = [x[..., k] for k in range(8)]
    tmp0, tmp7, tmp1, tmp6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    tmp2, tmp5, tmp3, tmp4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    sh = 11 if first else 15

    def ds(v, n):
        return (v + c(1 << (n - 1))) >> c(n)
    o = [None] * 8
    if first:
        o[0], o[4] = (tmp10 + tmp11) << c(2), (tmp10 - tmp11) << c(2)
    else:
        o[0], o[4] = ds(tmp10 + tmp11, 2), ds(tmp10 - tmp11, 2)
    z1 = (tmp12 + tmp13) * c(4433)
    o[2], o[6] = ds(z1 + tmp13 * c(6270), sh), ds(z1 - tmp12 * c(15137), sh)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * c(9633)
    tmp4, tmp5, tmp6, tmp7 = tmp4 * c(2446), tmp5 * c(16819), tmp6 * c(25172), tmp7 * c(12299)
    z1, z2, z3, z4 = z1 * c(-7373), z2 * c(-20995), z3 * c(-16069) + z5, z4 * c(-3196) + z5
    o[7], o[5], o[3], o[1] = ds(tmp4 + z1 + z3, sh), ds(tmp5 + z2 + z4, sh), ds(tmp6 + z2 + z3, sh), ds(tmp7 + z1 + z4, sh)
    return np.stack(o, axis=-1)


def component_planes(bgr, hs, vs):
    """-> [Y, Cb, Cr] int32 planes of bh[c] * 8 rows x bw[c] * 8 columns, as libjpeg hands them to the forward DCT"""
    h, w = bgr.shape[:2]
    g = jr.geometry(dict(hs=hs, vs=vs, ncomp=3), h, w)
    b, gg, r = (bgr[:, :, k].astype(np.int32) for k in range(3))
    y = (_fix(.299) * r + _fix(.587) * gg + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.168735892) * r - _fix(.331264108) * gg + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.418687589) * gg - _fix(.081312411) * b + (128 << 16) + 32767) >> 16
    out = [np.pad(y, ((0, g["bh"][0] * 8 - h), (0, g["bw"][0] * 8 - w)), "edge")]
    for c, p in ((1, cb), (2, cr)):
        p = np.pad(p, ((0, -(-h // vs) * vs - h), (0, g["bw"][c] * 8 * hs - w)), "edge")
        n = p.shape[1] // hs
        if (hs, vs) == (2, 1):
            p = (p[:, 0::2] + p[:, 1::2] + (np.arange(n) & 1)) >> 1
        elif (hs, vs) == (2, 2):
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 1 + (np.arange(n) & 1)) >> 2
        out.append(np.pad(p, ((0, g["bh"][c] * 8 - p.shape[0]), (0, 0)), "edge"))
    return out


def coefficients(bgr, quality=85, subsampling="420"):
    """-> (quantised coefficients int16 [n_blocks, 64], natural order, component planes one after the other as
    jpeg_ref.decode_coefficients gives them, dummy blocks resolved; descriptor)"""
    h, w = bgr.shape[:2]
    d = descriptor(h, w, quality, subsampling)
    hs, vs = d["hs"], d["vs"]
    g = jr.geometry(d, h, w)
    out = np.zeros((g["n_blocks"], 64), np.int16)
    for c, p in enumerate(component_planes(bgr, hs, vs)):
        bh, bw = g["bh"][c], g["bw"][c]
        blk = (p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128).astype(np.int32)
        blk = _fdct8(blk, True)                                                       # rows
        blk = _fdct8(blk.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)          # columns
        q8 = (d["qt"][d["tq"][c]].astype(np.int32) * 8).reshape(8, 8)
        blk = np.sign(blk) * ((np.abs(blk) + (q8 >> 1)) // q8)
        if c == 0:                                   # dummy blocks: no pixels, the DC of the block coded before them in the MCU
            nbx, nby = (w + 7) // 8, (h + 7) // 8
            m = blk.reshape(g["mcus_y"], vs, g["mcus_x"], hs, 64)
            dummy = (np.arange(bh) >= nby)[:, None] | (np.arange(bw) >= nbx)[None, :]
            dm = dummy.reshape(g["mcus_y"], vs, g["mcus_x"], hs)
            for j in range(1, hs * vs):
                v, hh, pv, ph = j // hs, j % hs, (j - 1) // hs, (j - 1) % hs
                sel = dm[:, v, :, hh]
                rep = np.zeros((g["mcus_y"], g["mcus_x"], 64), blk.dtype)
                rep[:, :, 0] = m[:, pv, :, ph, 0]
                m[:, v, :, hh] = np.where(sel[:, :, None], rep, m[:, v, :, hh])
            blk = m.reshape(bh, bw, 8, 8)
        out[g["off"][c]:g["off"][c] + bh * bw] = blk.reshape(-1, 64)
    return out, d


def scan_order(g, hs, vs):
    """-> (plane-layout block index, component) of every block in the order the scan codes them, int arrays [n_blocks]"""
    idx, comp = [], []
    mx, my = np.meshgrid(np.arange(g["mcus_x"]), np.arange(g["mcus_y"]))
    per = []
    for c in range(3):
        hsc, vsc = (hs, vs) if c == 0 else (1, 1)
        for v in range(vsc):
            for hh in range(hsc):
                per.append((g["off"][c] + (my * vsc + v) * g["bw"][c] + mx * hsc + hh, c))
    idx = np.stack([p[0].reshape(-1) for p in per], 1).reshape(-1)
    comp = np.tile(np.array([p[1] for p in per]), g["n_mcus"])
    return idx, comp


def scan_coefficients(coef, d, h, w):
    """The coefficients as the library's workspace holds them: int16 [n_blocks, 64] in scan order, each block in zigzag order."""
    g = jr.geometry(d, h, w)
    idx, _ = scan_order(g, d["hs"], d["vs"])
    return np.ascontiguousarray(coef[idx][:, jr.ZIGZAG])


def _codes(bits, vals):
    out, code, p = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            out[vals[p]] = (code, l)
            code += 1
            p += 1
        code <<= 1
    return out


DC_CODES = [_codes(jr.STD_DC_BITS[t], jr.STD_DC_VAL) for t in range(2)]
AC_CODES = [_codes(jr.STD_AC_BITS[t], jr.STD_AC_VAL[t]) for t in range(2)]


def header(h, w, quality=85, subsampling="420", restart_mcus=-1):
    """SOI .. the SOS header, as libjpeg writes them."""
    hs, vs = SUBSAMPLING[subsampling]
    g = jr.geometry(dict(hs=hs, vs=vs, ncomp=3), h, w)
    ri = interval_of(g, restart_mcus)
    qt = quant_tables(quality)
    o = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2):
        o += b"\xff\xdb\x00\x43" + bytes([t]) + qt[t][jr.ZIGZAG].tobytes()
    o += b"\xff\xc0\x00\x11\x08" + bytes([h >> 8, h & 255, w >> 8, w & 255, 3, 1, hs << 4 | vs, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc_th, bits, vals in ((0x00, jr.STD_DC_BITS[0], jr.STD_DC_VAL), (0x10, jr.STD_AC_BITS[0], jr.STD_AC_VAL[0]),
                              (0x01, jr.STD_DC_BITS[1], jr.STD_DC_VAL), (0x11, jr.STD_AC_BITS[1], jr.STD_AC_VAL[1])):
        n = 19 + len(vals)
        o += b"\xff\xc4" + bytes([n >> 8, n & 255, tc_th]) + bytes(bits) + bytes(vals)
    if ri:
        o += b"\xff\xdd\x00\x04" + bytes([ri >> 8, ri & 255])
    o += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    return bytes(o)


class _Writer:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 255)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        """Pad with 1-bits; -> the interval's bytes, unstuffed"""
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        out, self.out = bytes(self.out), bytearray()
        return out


def _encode_block(wr, zz, pred, t, stats):
    diff = int(zz[0]) - pred
    s = abs(diff).bit_length()
    wr.put(*DC_CODES[t][s])
    if s:
        wr.put((diff if diff >= 0 else diff - 1) & ((1 << s) - 1), s)
    stats["dc_cat"] = max(stats["dc_cat"], s)
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            wr.put(*AC_CODES[t][0xF0])
            stats["zrl"] += 1
            run -= 16
        s = abs(v).bit_length()
        wr.put(*AC_CODES[t][run << 4 | s])
        wr.put((v if v >= 0 else v - 1) & ((1 << s) - 1), s)
        stats["ac_cat"] = max(stats["ac_cat"], s)
        run = 0
    if run:
        wr.put(*AC_CODES[t][0])
    else:
        stats["no_eob"] += 1


def encode_scan(coef, d, h, w, restart_mcus=-1, stats=None):
    """coef as coefficients() gives them -> the entropy-coded data with its restart markers (between the SOS header and EOI)"""
    g = jr.geometry(d, h, w)
    ri = interval_of(g, restart_mcus)
    zz = scan_coefficients(coef, d, h, w)
    _, comp = scan_order(g, d["hs"], d["vs"])
    bpm = d["hs"] * d["vs"] + 2
    stats = stats if stats is not None else {}
    for k in ("dc_cat", "ac_cat", "zrl", "no_eob", "ff", "pad_bits"):
        stats.setdefault(k, 0 if k != "pad_bits" else set())
    out, wr, pred = bytearray(), _Writer(), [0, 0, 0]
    for m in range(g["n_mcus"]):
        if ri and m and m % ri == 0:
            stats["pad_bits"].add((8 - wr.n) % 8)
            seg = wr.flush()
            stats["ff"] += seg.count(b"\xff")
            out += seg.replace(b"\xff", b"\xff\x00") + bytes([0xFF, 0xD0 + (m // ri - 1) % 8])
            pred = [0, 0, 0]
        for j in range(bpm):
            b = m * bpm + j
            c = int(comp[b])
            _encode_block(wr, zz[b], pred[c], 1 if c else 0, stats)
            pred[c] = int(zz[b][0])
    stats["pad_bits"].add((8 - wr.n) % 8)
    seg = wr.flush()
    stats["ff"] += seg.count(b"\xff")
    return bytes(out + seg.replace(b"\xff", b"\xff\x00"))


def encode(bgr, quality=85, subsampling="420", restart_mcus=-1, stats=None):
    """BGR uint8 [h, w, 3] -> the frame's bytes"""
    h, w = bgr.shape[:2]
    coef, d = coefficients(bgr, quality, subsampling)
    return header(h, w, quality, subsampling, restart_mcus) + encode_scan(coef, d, h, w, restart_mcus, stats) + b"\xff\xd9"
