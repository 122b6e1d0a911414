"""NumPy restatement of the baseline-JPEG decoder of include/avhot.h (av_jpeg_parse / av_jpeg_decode): the header parse and the
restart-segment walk, the entropy decode with its lenient error rule and status bits, libjpeg's "islow" inverse DCT, the "fancy"
chroma upsampling and the colour conversion.  tests/golden/mjpeg.npz (Pillow's pixels) pins it; the library is then compared
with it, also on damaged streams, where no other decoder defines the answer.  Plus write_avi(), a tiny RIFF writer for the loader
tests."""
import struct

import numpy as np

ECODE, ERUN, EBYTES, ELEFT, ESEGS, EDESC = 1, 2, 4, 8, 16, 32
(E_TRUNCATED, E_FORMAT, E_SOF, E_ARITH, E_PRECISION, E_COMPONENTS, E_SAMPLING, E_DQT16, E_MULTISCAN, E_SIZE, E_TABLE, E_SCAN,
 E_SEGCAP) = range(-101, -114, -1)

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
                   49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# ITU-T T.81 Annex K.3
STD_DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
STD_DC_VAL = list(range(12))
STD_AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
STD_AC_VAL = (
    [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98,
     114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87,
     88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147,
     148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196,
     197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243,
     244, 245, 246, 247, 248, 249, 250],
    [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209,
     10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87,
     88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146,
     147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195,
     196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244,
     245, 246, 247, 248, 249, 250])


class JpegError(ValueError):
    def __init__(self, code, text):
        ValueError.__init__(self, text)
        self.code = code


def _bits_ok(bits, cap):
    code = n = 0
    for l in range(1, 17):
        code += bits[l - 1]
        n += bits[l - 1]
        if code > (1 << l):
            return False
        code <<= 1
    return n <= cap


def parse(data, h, w, seg_cap=1 << 30):
    """One frame's headers and its restart segments -> dict: width height ncomp hs vs restart_interval n_segments flags scan_offset
    tq td ta (per component), qt uint8 [4, 64] natural order, bits / vals {(class, slot): list}, segs [(begin, end)].  Raises
    JpegError with the library's AV_EJPEG_* code for what av_jpeg_parse refuses."""
    p, n_all = bytes(data), len(data)

    def fail(code, text):
        raise JpegError(code, text)
    if n_all < 2:
        fail(E_TRUNCATED, "ends before SOI")
    if p[0] != 0xFF or p[1] != 0xD8:
        fail(E_FORMAT, "no SOI")
    d = dict(width=0, height=0, ncomp=0, hs=0, vs=0, restart_interval=0, flags=0, tq=[0] * 4, td=[0] * 4, ta=[0] * 4,
             qt=np.zeros((4, 64), np.uint8), bits={}, vals={})
    pos, have_sof, have_q, comp_id = 2, False, set(), []
    while True:
        if pos + 2 > n_all:
            fail(E_TRUNCATED, "ends where a marker should be")
        if p[pos] != 0xFF:
            fail(E_FORMAT, "no marker where one should be")
        m = p[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        pos += 2
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            continue
        if m == 0xD9:
            fail(E_FORMAT, "EOI before any scan")
        if pos + 2 > n_all:
            fail(E_TRUNCATED, "ends inside a segment length")
        L = p[pos] * 256 + p[pos + 1]
        if L < 2:
            fail(E_FORMAT, "segment length below 2")
        if pos + L > n_all:
            fail(E_TRUNCATED, "ends inside a segment")
        seg = p[pos + 2:pos + L]
        n = L - 2
        pos += L
        if m == 0xC0:
            if have_sof:
                fail(E_FORMAT, "two frame headers")
            if n < 6:
                fail(E_FORMAT, "short SOF0")
            if seg[0] != 8:
                fail(E_PRECISION, "precision")
            nc = seg[5]
            if nc not in (1, 3):
                fail(E_COMPONENTS, "components")
            if n < 6 + 3 * nc:
                fail(E_FORMAT, "short SOF0")
            comp_id = []
            for c in range(nc):
                hv = seg[7 + 3 * c]
                comp_id.append(seg[6 + 3 * c])
                if seg[8 + 3 * c] > 3:
                    fail(E_TABLE, "quantiser selector")
                d["tq"][c] = seg[8 + 3 * c]
                if nc == 3 and (hv not in (0x11, 0x21, 0x22) if c == 0 else hv != 0x11):
                    fail(E_SAMPLING, "sampling")
                if c == 0:
                    d["hs"], d["vs"] = (hv >> 4, hv & 15) if nc == 3 else (1, 1)
            d["height"], d["width"], d["ncomp"] = seg[1] * 256 + seg[2], seg[3] * 256 + seg[4], nc
            if d["height"] != h or d["width"] != w:
                fail(E_SIZE, "size")
            have_sof = True
        elif m == 0xCC or 0xC9 <= m <= 0xCF:
            fail(E_ARITH, "arithmetic coding")
        elif 0xC1 <= m <= 0xC7 and m != 0xC4:
            fail(E_SOF, "not baseline")
        elif m == 0xC4:
            i = 0
            while i < n:
                if i + 17 > n:
                    fail(E_FORMAT, "short DHT")
                tc, th = seg[i] >> 4, seg[i] & 15
                if tc > 1 or th > 1:
                    fail(E_TABLE, "table class or slot")
                bits = list(seg[i + 1:i + 17])
                cnt = sum(bits)
                if not _bits_ok(bits, 256 if tc else 16):
                    fail(E_TABLE, "no prefix code")
                if i + 17 + cnt > n:
                    fail(E_FORMAT, "short DHT")
                vals = list(seg[i + 17:i + 17 + cnt])
                if not tc and any(v > 11 for v in vals):
                    fail(E_TABLE, "DC category above 11")
                d["bits"][(tc, th)], d["vals"][(tc, th)] = bits, vals
                i += 17 + cnt
        elif m == 0xDB:
            i = 0
            while i < n:
                if seg[i] >> 4:
                    fail(E_DQT16, "16-bit quantiser")
                tq = seg[i] & 15
                if tq > 3:
                    fail(E_TABLE, "quantiser slot")
                if i + 65 > n:
                    fail(E_FORMAT, "short DQT")
                d["qt"][tq][ZIGZAG] = np.frombuffer(seg[i + 1:i + 65], np.uint8)
                have_q.add(tq)
                i += 65
        elif m == 0xDD:
            if n < 2:
                fail(E_FORMAT, "short DRI")
            d["restart_interval"] = seg[0] * 256 + seg[1]
        elif m == 0xDA:
            break
    if not have_sof:
        fail(E_FORMAT, "scan before the frame header")
    nc = d["ncomp"]
    if n < 1 or seg[0] != nc:
        fail(E_MULTISCAN, "the scan does not hold every component")
    if n < 4 + 2 * nc:
        fail(E_FORMAT, "short SOS")
    have_dht = bool(d["bits"])
    for c in range(nc):
        if seg[1 + 2 * c] != comp_id[c]:
            fail(E_SCAN, "component order")
        td, ta = seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15
        if td > 1 or ta > 1:
            fail(E_TABLE, "table selector")
        d["td"][c], d["ta"][c] = td, ta
        if d["tq"][c] not in have_q:
            fail(E_TABLE, "quantiser missing")
        if have_dht and ((0, td) not in d["bits"] or (1, ta) not in d["bits"]):
            fail(E_TABLE, "Huffman table missing")
    sp = seg[1 + 2 * nc:]
    if sp[0] != 0 or sp[1] != 63 or sp[2] != 0:
        fail(E_SCAN, "not a sequential full scan")
    if not have_dht:
        for t in range(2):
            d["bits"][(0, t)], d["vals"][(0, t)] = list(STD_DC_BITS[t]), list(STD_DC_VAL)
            d["bits"][(1, t)], d["vals"][(1, t)] = list(STD_AC_BITS[t]), list(STD_AC_VAL[t])
    d["scan_offset"] = pos
    g = geometry(d, h, w)
    ri = d["restart_interval"]
    want = (g["n_mcus"] + ri - 1) // ri if ri > 0 else 1
    if want > seg_cap:
        fail(E_SEGCAP, "segment table too small")
    d["n_segments"] = want
    segs, q, first = [], pos, pos
    while q < n_all:
        if p[q] != 0xFF:
            nxt = p.find(b"\xff", q)
            q = n_all if nxt < 0 else nxt
            continue
        if q + 1 >= n_all:
            q = n_all
            break
        m = p[q + 1]
        if m == 0:
            q += 2
        elif 0xD0 <= m <= 0xD7:
            segs.append((first, q))
            q += 2
            first = q
        elif m == 0xD9:
            break
        elif m == 0xDA:
            fail(E_MULTISCAN, "a second scan")
        else:
            q += 1
    segs.append((first, q))
    if len(segs) != want:
        d["flags"] |= ESEGS
    segs = segs[:want] + [(q, q)] * (want - len(segs))
    d["segs"] = segs
    return d


def geometry(d, h, w):
    hs, vs, nc = d["hs"], d["vs"], d["ncomp"]
    mx, my = (w + 8 * hs - 1) // (8 * hs), (h + 8 * vs - 1) // (8 * vs)
    bw = [mx * (hs if c == 0 else 1) for c in range(nc)]
    bh = [my * (vs if c == 0 else 1) for c in range(nc)]
    off = [0]
    for c in range(nc):
        off.append(off[-1] + bw[c] * bh[c])
    return dict(mcus_x=mx, mcus_y=my, n_mcus=mx * my, bw=bw, bh=bh, off=off[:nc], n_blocks=off[-1], cw=(w + hs - 1) // hs, ch=(h + vs - 1) // vs)


def _table(bits, vals):
    """-> (look: 16-bit prefix -> (length, symbol) for codes up to 9 bits by dict of 9-bit prefixes, maxcode, valoff, vals[256])"""
    vals = (list(vals) + [0] * 256)[:256]
    look, maxcode, valoff, code, p = {}, [-1] * 18, [0] * 18, 0, 0
    for l in range(1, 17):
        n = bits[l - 1]
        valoff[l] = p - code
        if n > 0:
            if l <= 9:
                for k in range(n):
                    first = (code + k) << (9 - l)
                    for j in range(1 << (9 - l)):
                        look[first + j] = (l, vals[p + k])
            p += n
            code += n
            maxcode[l] = code - 1
        code <<= 1
    return look, maxcode, valoff, vals


class _Bits:
    """The readable bits of one segment: FF 00 is the byte FF, any other FF ends the data."""

    def __init__(self, seg):
        out, i, n = bytearray(), 0, len(seg)
        self.stopped = False
        while i < n:
            j = seg.find(b"\xff", i)
            if j < 0:
                out += seg[i:]
                break
            out += seg[i:j]
            if j + 1 < n and seg[j + 1] == 0:
                out.append(0xFF)
                i = j + 2
            else:
                self.stopped = True
                break
        self.nb = 8 * len(out)
        self.v = int.from_bytes(bytes(out) + b"\0\0", "big")       # 16 zero bits behind the data
        self.bp = 0

    def symbol(self, tab):
        look, maxcode, valoff, vals = tab
        avail = self.nb - self.bp
        w16 = (self.v >> (self.nb - self.bp)) & 0xFFFF if avail >= 0 else 0
        e = look.get(w16 >> 7)
        if e is not None:
            l, sym = e
        else:
            for l in range(10, 17):
                code = w16 >> (16 - l)
                if code <= maxcode[l]:
                    break
            else:
                return None, (EBYTES if avail < 16 else ECODE)
            sym = vals[(code + valoff[l]) & 255]
        if l > avail:
            return None, EBYTES
        self.bp += l
        return sym, 0

    def value(self, s):
        if self.nb - self.bp < s:
            return None, EBYTES
        u = (self.v >> (self.nb + 16 - self.bp - s)) & ((1 << s) - 1)
        self.bp += s
        return (u if u >= (1 << (s - 1)) else u - (1 << s) + 1), 0


def _block(r, dc, ac, pred, blk):
    sym, e = r.symbol(dc)
    if e:
        return pred, e
    sym &= 15
    if sym:
        v, e = r.value(sym)
        if e:
            return pred, e
        pred += v
    blk[0] = pred
    k = 1
    while k < 64:
        sym, e = r.symbol(ac)
        if e:
            return pred, e
        run, s = sym >> 4, sym & 15
        if s == 0:
            if run != 15:
                break
            if k + 16 > 64:
                return pred, ERUN
            k += 16
            continue
        k += run
        if k > 63:
            return pred, ERUN
        v, e = r.value(s)
        if e:
            return pred, e
        blk[ZIGZAG_L[k]] = v
        k += 1
    return pred, 0


ZIGZAG_L = ZIGZAG.tolist()


def decode_coefficients(data, h, w, d=None):
    """-> (coefficients int16 [n_blocks, 64] in natural order, component planes one after the other, status, descriptor)"""
    d = d or parse(data, h, w)
    g = geometry(d, h, w)
    p = bytes(data)
    coef = [[0] * 64 for _ in range(g["n_blocks"])]
    tabs = {k: _table(d["bits"][k], d["vals"][k]) for k in d["bits"]}
    status, ri, nc = d["flags"], d["restart_interval"], d["ncomp"]
    for i, (b, e_) in enumerate(d["segs"]):
        r = _Bits(p[b:e_])
        mcu0 = i * ri if ri > 0 else 0
        n = min(ri if ri > 0 else g["n_mcus"], g["n_mcus"] - mcu0)
        pred, err = [0, 0, 0], 0
        for m in range(mcu0, mcu0 + n):
            mx, my = m % g["mcus_x"], m // g["mcus_x"]
            for c in range(nc):
                hsc, vsc = (d["hs"], d["vs"]) if c == 0 else (1, 1)
                for v in range(vsc):
                    for hh in range(hsc):
                        blk = coef[g["off"][c] + (my * vsc + v) * g["bw"][c] + mx * hsc + hh]
                        pred[c], err = _block(r, tabs[(0, d["td"][c])], tabs[(1, d["ta"][c])], pred[c], blk)
                        if err:
                            blk[:] = [0] * 64
                            break
                    if err:
                        break
                if err:
                    break
            if err:
                break
        if not err and (r.nb - r.bp >= 8 or r.stopped):
            err = ELEFT
        status |= err
    return np.array(coef, np.int64).astype(np.int16).reshape(-1, 64), status, d


def _idct8(x, shift):
    """x: int32 [..., 8] along the last axis; wrapping 32-bit arithmetic."""
    i = [x[..., k] for k in range(8)]
    c = np.int32
    z1 = (i[2] + i[6]) * c(4433)
    tmp2, tmp3 = z1 - i[6] * c(15137), z1 + i[2] * c(6270)
    tmp0, tmp1 = (i[0] + i[4]) << c(13), (i[0] - i[4]) << c(13)
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * c(9633)
    tmp0, tmp1, tmp2, tmp3 = tmp0 * c(2446), tmp1 * c(16819), tmp2 * c(25172), tmp3 * c(12299)
    z1, z2, z3, z4 = z1 * c(-7373), z2 * c(-20995), z3 * c(-16069) + z5, z4 * c(-3196) + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    r = c(1 << (shift - 1))
    o = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([(v + r) >> c(shift) for v in o], axis=-1)


def idct_blocks(coef, q):
    """coef int16 [n, 64], q uint8 [64] -> uint8 [n, 8, 8]"""
    with np.errstate(over="ignore"):
        x = (coef.astype(np.int32) * q.astype(np.int32)).reshape(-1, 8, 8)
        ws = _idct8(x.transpose(0, 2, 1), 11).transpose(0, 2, 1)          # columns first
        out = _idct8(ws, 18)
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def _planes(coef, d, g):
    out = []
    for c in range(d["ncomp"]):
        n = g["bw"][c] * g["bh"][c]
        b = idct_blocks(coef[g["off"][c]:g["off"][c] + n], d["qt"][d["tq"][c]])
        out.append(b.reshape(g["bh"][c], g["bw"][c], 8, 8).transpose(0, 2, 1, 3).reshape(g["bh"][c] * 8, g["bw"][c] * 8))
    return out


def _h2(t, r0, r1, sh):
    """triangle filter along x: t int32 [rows, cw] -> [rows, 2 cw]"""
    left, right = np.concatenate([t[:, :1], t[:, :-1]], 1), np.concatenate([t[:, 1:], t[:, -1:]], 1)
    out = np.empty((t.shape[0], 2 * t.shape[1]), np.int32)
    out[:, 0::2] = (3 * t + left + r0) >> sh
    out[:, 1::2] = (3 * t + right + r1) >> sh
    return out


def upsample(plane, hs, vs, h, w):
    """chroma plane (MCU-padded) -> int32 [h, w]: libjpeg's fancy upsampling over the real extent"""
    cw, ch = (w + hs - 1) // hs, (h + vs - 1) // vs
    s = plane[:ch, :cw].astype(np.int32)
    if hs == 1:
        return s[:h, :w]
    if vs == 1:
        return _h2(s, 1, 2, 2)[:h, :w]
    up, dn = np.concatenate([s[:1], s[:-1]], 0), np.concatenate([s[1:], s[-1:]], 0)
    t = np.empty((2 * ch, cw), np.int32)
    t[0::2], t[1::2] = 3 * s + up, 3 * s + dn
    return _h2(t, 8, 7, 4)[:h, :w]


def pixels(coef, d, h, w):
    g = geometry(d, h, w)
    pl = _planes(coef, d, g)
    y = pl[0][:h, :w].astype(np.int32)
    if d["ncomp"] == 1:
        return np.repeat(y[:, :, None], 3, 2).astype(np.uint8)
    cb, cr = upsample(pl[1], d["hs"], d["vs"], h, w) - 128, upsample(pl[2], d["hs"], d["vs"], h, w) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    gg = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([b, gg, r], 2), 0, 255).astype(np.uint8)


def decode(data, h, w):
    """-> (BGR uint8 [h, w, 3], status)"""
    coef, status, d = decode_coefficients(data, h, w)
    return pixels(coef, d, h, w), status


def damaged_variants(data, h, w, n_flips=200, seed=0):
    """The damaged versions of one frame the lenient decode is checked on, as (name, bytes): 16 truncations, n_flips seeded one-byte
    corruptions inside the scan, a scan of FF 00 repeated, a scan of zeros."""
    data = bytes(data)
    so = parse(data, h, w)["scan_offset"]
    out = [("cut%d" % k, data[:len(data) * (k + 1) // 17]) for k in range(16)]
    rng = np.random.RandomState(seed)
    for k in range(n_flips):
        pos, val = int(rng.randint(so, len(data) - 2)), int(rng.randint(0, 256))
        out.append(("flip%d" % k, data[:pos] + bytes([val]) + data[pos + 1:]))
    n = len(data) - 2 - so
    out.append(("ff00", data[:so] + (b"\xff\x00" * n)[:n] + data[-2:]))
    out.append(("zeros", data[:so] + b"\0" * n + data[-2:]))
    return out


# ---- a tiny RIFF / AVI writer -------------------------------------------------------------------------------------------------
def _chunk(cc, payload):
    return cc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def write_avi(path, jpegs, fps, w, h, idx1=True, handler=b"MJPG", junk=False, absolute_index=False):
    """AVI 1.0 with one MJPG video stream: hdrl (avih, strl: strh + strf), optionally a JUNK chunk, movi with one 00dc chunk per
    frame, and idx1 (offsets relative to the 'movi' tag, or absolute file offsets)."""
    n, rate, scale = len(jpegs), int(round(fps * 1000)), 1000
    avih = struct.pack("<14I", int(round(1e6 / fps)), 0, 0, 0x10 if idx1 else 0, n, 0, 1, max(map(len, jpegs)), w, h, 0, 0, 0, 0)
    strh = b"vids" + handler + struct.pack("<IHHIIIIIIII4h", 0, 0, 0, 0, scale, rate, 0, n, max(map(len, jpegs)), 0xFFFFFFFF, 0, 0, 0, w, h)
    strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, handler, w * h * 3, 0, 0, 0, 0)
    hdrl = b"LIST" + struct.pack("<I", 0) + b"hdrl" + _chunk(b"avih", avih) + b"LIST"
    strl = b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf)
    hdrl += struct.pack("<I", len(strl)) + strl
    hdrl = hdrl[:4] + struct.pack("<I", len(hdrl) - 8) + hdrl[8:]
    head = b"RIFF" + struct.pack("<I", 0) + b"AVI " + hdrl
    if junk:
        head += _chunk(b"JUNK", b"\0" * 37)
    movi, index = b"movi", []
    for k, j in enumerate(jpegs):
        if junk and k == 1:
            movi += _chunk(b"JUNK", b"\0" * 10)
        index.append((len(movi), len(j)))
        movi += _chunk(b"00dc", bytes(j))
    movi_tag = len(head) + 8
    body = head + b"LIST" + struct.pack("<I", len(movi)) + movi
    if idx1:
        base = movi_tag if absolute_index else 0
        body += _chunk(b"idx1", b"".join(b"00dc" + struct.pack("<III", 0x10, base + o, s) for o, s in index))
    body = body[:4] + struct.pack("<I", len(body) - 8) + body[8:]
    with open(path, "wb") as f:
        f.write(body)
